"""CPU: the reference of the maximal repeats (tests/maxrep_ref.py: the capped LCP array of repeat_ref plus a stack) against a brute
force from the definition and against the answers that are known; the per-row rule and the host's share of the selection
(bce_amd/csrc/maxrep_step.h) compiled by g++ into a stand-alone program under ASan + UBSan (tests/maxrep_emul.cpp) and driven with
blocks of 4 and 8 rows; the new symbols and names, and the refusals that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bce_amd
from bce_amd import api
from conftest import ROOT

import maxrep_ref as ref
import repeat_ref

SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
NAMED = [b"a", b"aa", b"ab", b"abab", b"aaaa", b"abcXabc", b"abracadabra", b"abracadabra" * 3, b"mississippi", b"banana", b"abcabcabd"]
BOUNDS = (1, 2, 3, 8, 64)
KNOWN = [  # text, max_len, (len, count, row) by length, BWT runs
    (b"abracadabra", 64, [(4, 2, 1), (1, 5, 0)], 7),
    (b"mississippi", 64, [(4, 2, 2), (1, 4, 0), (1, 4, 7), (1, 2, 5)], 8),
    (b"abcXabc", 64, [(3, 2, 1)], 4),
    (b"abab", 64, [], 2),
    (b"abracadabra" * 3, 8, [(4, 6, 3), (1, 15, 0)], 7),
]


def _texts():
    rs = np.random.RandomState(11)
    texts = list(NAMED)
    for i in range(120):
        n, k = int(rs.randint(1, 41)), 1 + i % 4
        texts.append(bytes(rs.randint(97, 97 + k, n).astype(np.uint8)))
    return texts


def _arrays(t, L):
    sa = ref.rotation_order(t)
    return repeat_ref.capped_lcp(t, L), sa, ref.bwt_of(t, sa)


def test_the_rotation_order_sorts_the_rotations():
    for t in _texts():
        sa = ref.rotation_order(t).tolist()
        rots = [t[i:] + t[:i] for i in sa]
        assert sorted(sa) == list(range(len(t))) and rots == sorted(rots), t


def test_the_lcp_array_of_an_order_is_the_capped_array_of_the_windows():
    for t in _texts() + [b"ab" * 700, bce_amd.synth_text(3, 3000).tobytes()]:
        for L in (1, 3, 64, 1500):
            assert np.array_equal(ref.lcp_of_order(t, ref.rotation_order(t), L), repeat_ref.capped_lcp(t, L)), (t[:40], L)


def test_the_stack_reference_is_the_brute_force_set():
    total = 0
    for t in _texts():
        n = len(t)
        for L in BOUNDS:
            lcp, sa, bw = _arrays(t, L)
            found = ref.intervals(lcp, bw)
            assert len(set(x[:3] for x in found)) == len(found), (t, L)          # every interval once
            for min_len in (1, 2, 3):
                if min_len > L:
                    continue
                got = set((l, c, p, bytes(t[(int(sa[p]) + j) % n] for j in range(l))) for l, c, p, _ in found if l >= min_len)
                assert got == ref.brute_force(t, min_len, L), (t, L, min_len)
                total += len(got)
            for l, c, p, r in found:
                assert (l < n or l == L) and c >= 2 and p < r < p + c <= n, (t, L)
    assert total > 1000


def test_the_known_answers():
    for t, L, want, runs in KNOWN:
        ents, info = ref.of_text(t, 1, L, "len", 100)
        assert ents == want and info == {"total": len(want), "capped": 0, "bwt_runs": runs, "found": len(want)}, (t, ents, info)
    assert ref.of_text(b"a", 1, 64, "len", 5) == ([], {"total": 0, "capped": 0, "bwt_runs": 1, "found": 0})
    assert ref.of_text(b"abracadabra" * 3, 1, 8, "count", 1)[0] == [(1, 15, 0)]
    assert ref.of_text(b"abracadabra" * 3, 2, 8, "gain", 9)[0] == [(4, 6, 3)]
    ents, info = ref.of_text(b"abcdefgh" + b"xy" + b"abcdefgh" + b"z", 1, 4, "len", 9)   # a repeat of 8 bytes at the bound 4: "4 or more"
    assert info["capped"] == 1 and ents[0][:2] == (4, 2)


def test_the_orders_and_their_ties():
    t = b"mississippi"
    assert ref.of_text(t, 1, 64, "count", 9)[0] == [(1, 4, 0), (1, 4, 7), (4, 2, 2), (1, 2, 5)]
    assert ref.of_text(t, 1, 64, "gain", 9)[0] == [(4, 2, 2), (1, 4, 0), (1, 4, 7), (1, 2, 5)]   # gain 3 twice: rows ascending
    assert [ref.weight(o, 4096, (1 << 31) - 1) < 1 << 44 for o in ("len", "count", "gain")] == [True] * 3
    assert ref.weight("gain", 4096, (1 << 20) + 1) == 1 << 32


# ---- maxrep_step.h on the host ---------------------------------------------------------------------------------------------------

def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "maxrep_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "maxrep_emul.cpp")])
    return exe


def _run(emul, path, from_stdin=False):
    with open(path) as f:
        r = subprocess.run([emul] if from_stdin else [emul, str(path)], stdin=f if from_stdin else None, capture_output=True, text=True, env=SAN_ENV)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def _words(v):
    return ",".join(str(int(x)) for x in v) if len(v) else "-"


def test_the_row_rule_in_blocks_of_4_and_8_rows_gives_the_reference_list(tmp_path):
    emul = _build_emul()
    rs = np.random.RandomState(3)
    cases = []
    for t in _texts():
        for L in (1, 3, 64):
            lcp, sa, bw = _arrays(t, L)
            for B, min_len, order, limit in ((4, 1, 0, 1000), (8, 1, 2, 3), (4, min(2, L), 1, 1)):
                cases.append((B, min_len, L, order, limit, lcp, bw))
    for i in range(60):                                                        # arrays that are no text's: any words, any bytes
        n = int(rs.randint(1, 70))
        lcp = rs.randint(0, 1 + (1, 2, 5, 4096)[i % 4], n)
        lcp[0] = 0
        bw = rs.randint(0, 2 + i % 3, n)
        cases.append((4 + 4 * (i % 2), 1 + i % 2, 4096, i % 3, (1, 5, 1000)[i % 3], lcp, bw))
    n = 37                                                                     # a word of 0xFFFFFFFF names no interval
    lcp = np.array([0] + [3, 0xFFFFFFFF, 3, 1] * 9, dtype=np.uint64)
    cases.append((4, 1, 4096, 0, 100, lcp, np.arange(n) % 2))
    src = tmp_path / "rows.txt"
    src.write_text("".join("rows %d %d %d %d %d %s %s\n" % (B, m, L, o, lim, _words(lcp), _words(bw)) for B, m, L, o, lim, lcp, bw in cases))
    for from_stdin in (False, True):
        r = _run(emul, src, from_stdin)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        for (B, m, L, o, lim, lcp, bw), line in zip(cases, lines):
            w = line.split()
            want = [x for x in ref.intervals(lcp, bw) if x[0] >= m]
            want.sort(key=lambda x: (-ref.weight(o, x[0], x[1]), x[3]))
            got = [] if w[5] == "-" else [tuple(int(v) for v in e.split(":")) for e in w[5].split(",")]
            assert w[0] == "rows" and got == want[:lim], (B, m, L, o, lim, list(lcp), list(bw), line)
            assert [int(v) for v in w[1:5]] == [len(want), sum(1 for x in want if x[0] == L), ref.bwt_runs(bw), min(lim, len(want))], line


def _weight_lists():
    rs = np.random.RandomState(7)
    lists = [[1], [5], [7] * 9, [4, 5, 6, 7] * 3,                            # one repeat; all equal; one bin only: every repeat is a candidate
             [1, 2, 3, 4, 5, 6, 7, 8, 9], [9, 8, 7, 6, 5, 4, 3, 2, 1], [2, 1, 2, 1, 3, 3, 2],
             [1 << 32, (1 << 32) - 1, 1, (1 << 32) + 1, 1 << 31, 1 << 33, (1 << 32) - 1, 1 << 32],   # both sides of 2^32
             [(4096 << 31) | 5, (4096 << 31) | 4, (1 << 31) | 2, (17 << 31) | 2, (4096 << 31) | 5], [(1 << 44) - 1, 1 << 43, 1],
             [(1 << 64) - 1, 1 << 63, 1 << 62, 3], [1000] + [1] * 40, [3] * 5 + [2] * 5 + [64, 65, 127, 128]]
    for i in range(40):
        m = int(rs.randint(1, 60))
        lists.append([int(v % (1 << (1 + i % 43))) + 1 for v in rs.zipf(1.3, m)])   # Zipf-distributed
    return lists


def test_the_threshold_keeps_every_member_of_the_list_for_every_limit(tmp_path):
    emul = _build_emul()
    cases = [(limit, ws) for ws in _weight_lists() for limit in list(range(1, len(ws) + 3)) + [1 << 20]]
    src = tmp_path / "sel.txt"
    src.write_text("".join("sel %d %s\n" % (limit, _words(ws)) for limit, ws in cases))
    r = _run(emul, src)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for (limit, ws), line in zip(cases, lines):
        w = line.split()
        t, cand, top, bits, found = (int(v) for v in w[1:6])
        got = [int(v) for v in w[6].split(",")]
        want = sorted(range(len(ws)), key=lambda i: (-ws[i], i))[:limit]       # the true list
        assert w[0] == "sel" and found == len(want) == min(limit, len(ws)) and got == want, (limit, ws, line)
        assert (t, cand, got) == ref.select(ws, limit)
        hist = [sum(1 for x in ws if x.bit_length() - 1 == b) for b in range(64)]
        assert cand == sum(hist[t:]) >= found and top == max(x.bit_length() for x in ws) - 1
        assert sum(hist[t + 1:]) < found                                       # the largest such bin: one higher loses a member
        assert ws[want[-1]] >= 1 << t                                          # the last member is a candidate, so every member is
        assert bits == ((1 << (top + 1)) - 1 - (1 << t)).bit_length()
        if len(set(x.bit_length() for x in ws)) == 1:                          # one bin: every repeat is a candidate
            assert cand == len(ws)


def test_the_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("x\n", "sel 0 1\n", "sel 1 0\n", "sel 1 1x\n", "rows 5 1 4 0 1 0 0\n", "rows 4 0 4 0 1 0 0\n", "rows 4 1 4 3 1 0 0\n",
                 "rows 4 1 4 0 1 0,1 0\n", "rows 4 1 4 0 0 0 0\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        assert _run(emul, src).returncode == 3, text


# ---- ABI, names, refusals without a device ----------------------------------------------------------------------------------------

NEW = {"bce_hip_maximal_repeats": 10, "bce_hip_maximal_repeats_device": 10, "bce_hip_maxrep_of_arrays_device": 11}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert re.search(r"typedef struct bce_hip_maxrep \{\s*uint32_t len, count, row, pos;\s*\} bce_hip_maxrep;", src)
    assert api.MAXREP_DTYPE.names == ("len", "count", "row", "pos") and api.MAXREP_DTYPE.itemsize == 16
    assert [n for n, _ in api.MaxRepInfo._fields_] == ["total", "capped", "bwt_runs", "found", "reserved"] and C.sizeof(api.MaxRepInfo) == 32
    for name, value in (("LEN", 0), ("COUNT", 1), ("GAIN", 2)):
        assert re.search(r"#define\s+BCE_HIP_MAXREP_BY_%s\s+%du" % (name, value), src) and api.MAXREP_ORDERS[name.lower()] == value
    for name in ("maximal_repeats", "maximal_repeats_tensor", "maximal_repeats_in_archive", "maxrep_of_arrays_device", "MaxRepInfo"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("maximal_repeats", "maximal_repeats_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name


def test_a_null_context_is_refused_and_leaves_the_outputs_untouched():
    lib = bce_amd.load_library()
    out = np.full(4, 7, dtype=api.MAXREP_DTYPE)
    raw = np.full(32, 9, dtype=np.uint8)
    info = api.MaxRepInfo(1, 2, 3, 4, 5)
    for args in ((1, 64, 0, 4), (0, 64, 0, 4), (1, 4097, 0, 4), (1, 64, 3, 4), (1, 64, 0, 0)):
        assert lib.bce_hip_maximal_repeats(None, *args, out.ctypes.data, raw.ctypes.data, 8, 32, C.byref(info)) == -1
        assert lib.bce_hip_maximal_repeats_device(None, *args, out.ctypes.data, raw.ctypes.data, 8, 32, C.byref(info)) == -1
        assert lib.bce_hip_maxrep_of_arrays_device(None, raw.ctypes.data, 8, raw.ctypes.data, raw.ctypes.data, *args, out.ctypes.data, C.byref(info)) == -1
    assert (out == np.full(4, 7, dtype=api.MAXREP_DTYPE)).all() and (raw == 9).all()
    assert (info.total, info.capped, info.bwt_runs, info.found, info.reserved) == (1, 2, 3, 4, 5)


def test_python_refuses_an_unknown_order_and_numbers_that_are_no_uint32():
    for args in ((-1, 1, "len", 1, 0), (1, 1 << 32, "len", 1, 0), (1, 1, "size", 1, 0), (1, 1, 0, -1, 0), (1, 1, 0, 1, 1 << 32)):
        try:
            api._maxrep_args(*args)
        except ValueError:
            continue
        raise AssertionError(args)
    assert api._maxrep_args(np.uint32(2), np.int64(64), "gain", 100, 5) == [2, 64, 2, 100, 5]
    assert api._maxrep_args(1, 4096, 1, 1, 0) == [1, 4096, 1, 1, 0]
