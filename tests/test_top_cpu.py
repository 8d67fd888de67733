"""CPU: the references of the most frequent k-grams (tests/top_ref.py) against the counted classes of tests/repeat_ref.py and against
each other; the host's share of the selection (bce_amd/csrc/top_step.h: the bin, the threshold, the sort key, the escape) compiled
by g++ into a stand-alone program under ASan + UBSan (tests/top_emul.cpp); the new symbols and names, and the refusals that need
no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import bce_amd
from bce_amd import api
from conftest import ROOT

import locate_ref
import repeat_ref
import top_ref as ref
from test_count_cpu import _texts

SAN_ENV = dict(os.environ, ASAN_OPTIONS="abort_on_error=0:detect_leaks=1:exitcode=99", UBSAN_OPTIONS="halt_on_error=1:exitcode=98")
KS = (0, 1, 2, 3, 5, 8, 45)


def test_the_reference_counts_the_classes_of_the_kgram_reference():
    texts, _ = _texts()
    for t in texts:
        for k in KS:
            ents, distinct, hist = ref.top_kgrams(t, k, 1 << 20)
            sizes = repeat_ref.kgram_classes(t, k)
            assert sorted(c for c, _, _ in ents) == sizes and distinct == len(sizes) and sum(hist) == distinct, (t, k)
            assert hist == [sum(1 for s in sizes if s.bit_length() - 1 == b) for b in range(32)]
            assert [c for c, _, _ in ents] == sorted(sizes, reverse=True)
            n = len(t)
            for c, row, g in ents:                                           # the k-gram is one, counted cyclically, and its row a row
                assert len(g) == k and 0 <= row <= n - c and sum((t * (k // n + 2))[i:i + k] == g for i in range(n)) == c
            for limit in (1, 2, distinct):
                assert ref.top_kgrams(t, k, limit)[0] == ents[:limit]
    assert ref.top_kgrams(b"abracadabra", 2, 3) == ([(2, 1, b"ab"), (2, 5, b"br"), (2, 9, b"ra")], 8, [5, 3] + [0] * 30)
    assert ref.top_kgrams(b"z", 7, 5) == ([(1, 0, b"zzzzzzz")], 1, [1] + [0] * 31)
    assert ref.top_kgrams(b"ab" * 150, 3, 9)[0] == [(150, 0, b"aba"), (150, 150, b"bab")]


def test_the_tie_order_is_the_row_order_of_the_classes_of_the_lcp_array():
    """The list from the text alone (ties by the bytes) is the list from the LCP array of the sorted rotations (ties by the first
    row): rows are sorted rotations, so a lower first row is a smaller k-gram."""
    texts, _ = _texts()
    for t in texts:
        sa = locate_ref.suffix_array_of_rotations(t)
        for k in KS:
            lcp = repeat_ref.lcp_of_order(t, sa, max(k, 1))
            for limit in (1, 3, len(t) + 1):
                ents, distinct, hist = ref.top_kgrams(t, k, limit)
                counts, rows, d2, h2 = ref.top_of_lcp(lcp, k, limit)
                assert (counts.tolist(), rows.tolist(), d2, h2) == ([c for c, _, _ in ents], [r for _, r, _ in ents], distinct, hist), (t, k, limit)
                n = len(t)
                for (c, row, g) in ents:                                     # the rotation in the class's first row starts with the k-gram
                    assert bytes(t[(sa[row] + j) % n] for j in range(k)) == g


def _build_emul():
    exe = os.path.join(ROOT, "tests", "_build", "top_emul")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                           "-o", exe, os.path.join(ROOT, "tests", "top_emul.cpp")])
    return exe


def _run(emul, path, from_stdin=False):
    with open(path) as f:
        r = subprocess.run([emul] if from_stdin else [emul, str(path)], stdin=f if from_stdin else None, capture_output=True, text=True, env=SAN_ENV)
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    return r


def _size_lists():
    rs = np.random.RandomState(7)
    lists = [[1], [5], [1] * 9, [4, 5, 6, 7] * 3,                          # one class; one bin only: every class is a candidate
             [1, 2, 3, 4, 5, 6, 7, 8, 9], [9, 8, 7, 6, 5, 4, 3, 2, 1], [2, 1, 2, 1, 3, 3, 2],
             [1 << 30, 1, (1 << 31) - 1, 1 << 30], [(1 << 31) - 1], [1000] + [1] * 40, [3] * 5 + [2] * 5 + [64, 65, 127, 128]]
    for i in range(40):
        m = int(rs.randint(1, 60))
        lists.append([int(v) for v in (rs.zipf(1.3, m) % (1 << (1 + i % 20))) + 1])
    return lists


def test_the_threshold_keeps_every_member_of_the_list_for_every_limit(tmp_path):
    emul = _build_emul()
    cases = [(limit, sizes) for sizes in _size_lists() for limit in list(range(1, len(sizes) + 3)) + [1 << 20]]
    src = tmp_path / "cases.txt"
    src.write_text("".join("s %d %d %s\n" % (limit, len(sizes), " ".join(map(str, sizes))) for limit, sizes in cases))
    for from_stdin in (False, True):
        r = _run(emul, src, from_stdin)
        assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
        lines = r.stdout.splitlines()
        assert len(lines) == len(cases)
        for (limit, sizes), line in zip(cases, lines):
            w = line.split()
            t, cand, top, bits, found = (int(v) for v in w[1:6])
            got = [tuple(int(v) for v in p.split(":")) for p in w[6:]]
            want = sorted(((s, i) for i, s in enumerate(sizes)), key=lambda p: (-p[0], p[1]))[:limit]
            assert w[0] == "s" and found == len(want) == min(limit, len(sizes)) and got == want, (limit, sizes, line)
            hist = ref.size_hist(sizes)
            assert cand == sum(1 for s in sizes if s >= 1 << t) == sum(hist[t:]) >= found and top == max(s.bit_length() for s in sizes) - 1
            assert sum(hist[t + 1:]) < found                                # the largest such bin: one higher loses a member
            assert want[-1][0] >= 1 << t                                    # the last member is a candidate, so every member is
            assert bits == ((1 << (top + 1)) - 1 - (1 << t)).bit_length() and (bits == 0) == (top == t == 0)
            if len(set(s.bit_length() for s in sizes)) == 1:                 # one bin: every class is a candidate
                assert cand == len(sizes)


def test_the_escape_is_printable_ascii_or_hex(tmp_path):
    emul = _build_emul()
    src = tmp_path / "e.txt"
    src.write_text("e\n")
    r = _run(emul, src)
    assert r.returncode == 0
    w = r.stdout.split()
    assert w[0] == "e" and w[1:] == [ref.escape(bytes([b])) for b in range(256)]
    assert ref.escape(b"a b\\c\x00\x7f~!\xff") == "a\\x20b\\x5Cc\\x00\\x7F~!\\xFF"
    assert all(len(e) in (1, 4) and " " not in e for e in w[1:]) and w[1 + 0x5C] == "\\x5C" and w[1 + 0x20] == "\\x20" and w[1 + 0x41] == "A"


def test_the_emulator_refuses_malformed_input(tmp_path):
    emul = _build_emul()
    for text in ("x\n", "s 0 1 1\n", "s 1 0\n", "s 1 2 1\n", "s 1 1 0\n", "s 1 1 2147483648\n", "s 1 1 1x\n"):
        src = tmp_path / "bad.txt"
        src.write_text(text)
        assert _run(emul, src).returncode == 3, text


# ---- ABI, names, refusals without a device ----------------------------------------------------------------------------------------

NEW = {"bce_hip_top_kgrams": 9, "bce_hip_top_kgrams_device": 9, "bce_hip_top_classes_of_lcp_device": 10}


def test_the_new_symbols_are_exported_declared_and_bound():
    lib = C.CDLL(bce_amd.library_path())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bce_hip.h")).read(), flags=re.S)
    bound = {n: (r, a) for n, r, a in api.SYMBOLS}
    for name, nargs in NEW.items():
        assert hasattr(lib, name), name
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % name, src)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert name in bound and bound[name][0] is C.c_int and len(bound[name][1]) == nargs, name
    assert re.search(r"typedef struct bce_hip_top_kgram \{\s*uint32_t count, row, pos;\s*\} bce_hip_top_kgram;", src)
    assert [n for n, _ in api.TopKGram._fields_] == ["count", "row", "pos"] and C.sizeof(api.TopKGram) == 12 == api.TOP_DTYPE.itemsize
    assert api.TOP_DTYPE.names == ("count", "row", "pos")
    assert re.search(r"#define\s+BCE_HIP_TOP_MAX\s+\(1u << 20\)", src) and api.TOP_MAX == 1 << 20
    for name in ("top_kgrams", "top_kgrams_tensor", "top_kgrams_in_archive", "top_classes_of_lcp_device", "TopKGram", "TopKGrams"):
        assert callable(getattr(bce_amd, name)), name
    for name in ("top_kgrams", "top_kgrams_device"):
        assert callable(getattr(bce_amd.RankFile, name)), name


def test_a_null_context_is_refused_and_leaves_the_outputs_untouched():
    lib = bce_amd.load_library()
    out, raw = (api.TopKGram * 4)(), (C.c_uint8 * 32)(*([9] * 32))
    for e in out:
        e.count, e.row, e.pos = 11, 12, 13
    found, distinct, hist = C.c_uint32(5), C.c_uint64(6), (C.c_uint64 * 32)(*([7] * 32))
    tail = (C.byref(found), C.byref(distinct), C.addressof(hist))
    for k, limit, cap in ((2, 4, 32), (4097, 4, 32), (2, 0, 32), (2, (1 << 20) + 1, 32), (8, 4, 31), (0, 1, 0)):
        assert lib.bce_hip_top_kgrams(None, k, limit, C.addressof(out), C.addressof(raw), cap, *tail) == -1
        assert lib.bce_hip_top_kgrams_device(None, k, limit, C.addressof(out), C.addressof(raw), cap, *tail) == -1
        assert lib.bce_hip_top_classes_of_lcp_device(None, C.addressof(raw), 8, C.addressof(raw), k, limit, C.addressof(out), *tail) == -1
    assert all((e.count, e.row, e.pos) == (11, 12, 13) for e in out) and list(raw) == [9] * 32
    assert (found.value, distinct.value, list(hist)) == (5, 6, [7] * 32)


def test_python_refuses_numbers_that_are_no_uint32_before_the_library():
    for k, limit in ((-1, 1), (1, -1), (1 << 32, 1), (1, 1 << 32)):
        try:
            api._top_limit(k, limit)
        except ValueError:
            continue
        raise AssertionError((k, limit))
    assert api._top_limit(np.uint32(8), np.int64(100)) == (8, 100)
    t = api.TopKGrams([(2, 0, 0, b"ab")], 8, [5, 3] + [0] * 30)
    assert t == [(2, 0, 0, b"ab")] and t.distinct == 8 and t.size_hist[:2] == [5, 3] and len(t.size_hist) == 32
