"""CPU: the host references of the suffix-array tests (tests/sa_ref.py) against definitions that cannot be wrong -- Python's sort of the
suffixes, a loop over the checker's three stages -- and against the reference project's build, through the BWT read off the array."""
import itertools

import numpy as np
import pytest

import oracle
import sa_ref


def brute(t):
    t = bytes(t)
    return np.array(sorted(range(len(t)), key=lambda i: t[i:]), dtype=np.int32)


def check_by_loops(t, sa):
    """bce_hip_sufcheck's definition (include/bce_hip.h), word for word."""
    t, n = bytes(t), len(t)
    sa = [int(x) & 0xFFFFFFFF for x in sa]
    for i, p in enumerate(sa):
        if p >= n:
            return sa_ref.RANGE, i
    named = set(sa)
    for p in range(n):
        if p not in named:
            return sa_ref.MISSING, p
    inv = {p: i for i, p in enumerate(sa)}
    for i in range(1, n):
        a, b = sa[i - 1], sa[i]
        if t[a] < t[b]:
            continue
        if t[a] == t[b] and (a + 1 == n or (b + 1 < n and inv[a + 1] < inv[b + 1])):
            continue
        return sa_ref.ORDER, i
    return sa_ref.OK, sa_ref.NONE


def small_strings():
    rs = np.random.RandomState(17)
    out = [b"a", b"ab", b"ba", b"aa", b"aaa", b"abracadabra", b"banana", b"\x00\x00\x01\x00", b"\xff" * 7, b"ab" * 9, bytes(range(256))]
    for _ in range(300):
        n = int(rs.randint(1, 80))
        out.append(bytes(rs.choice([0, 1, 97, 98, 255], n).astype(np.uint8)))
    return out


def test_the_reference_array_is_the_sorted_suffixes():
    for t in small_strings():
        assert (sa_ref.suffix_array(t) == brute(t)).all(), t
    # the doubling route (300 bytes and more) against the same sort, ties of every depth included
    for t in (oracle.synth_text(1, 3000), oracle.synth_rand(2, 1000), b"a" * 700, b"ab" * 400 + b"a", b"abc" * 333 + b"ab", bytes(2000),
              oracle.synth_text(3, 500) * 4):
        sa = sa_ref.suffix_array(t)
        assert (sa == brute(t)).all()
        assert (sa_ref.inverse(sa)[sa] == np.arange(len(t))).all()


def test_the_rule_passes_exactly_the_sorted_permutation():
    """Every permutation of the rows of short strings: check() accepts the suffix array and nothing else."""
    for t in (b"a", b"ab", b"aa", b"aab", b"aba", b"aaaa", b"abab", b"banan", b"aabaa", b"\x00\x00\x01\x00\x00", b"abcab", b"aaaaa", b"mississ"[:6]):
        want = list(brute(t))
        for perm in itertools.permutations(range(len(t))):
            got = sa_ref.check(t, np.array(perm, dtype=np.uint32))
            assert (got == (sa_ref.OK, sa_ref.NONE)) == (list(perm) == want), (t, perm, got)
            assert got == check_by_loops(t, perm)


def test_check_on_sound_arrays():
    for t in small_strings() + [oracle.synth_text(1, 5000), oracle.synth_rand(2, 4099), b"a" * 5000, b"ab" * 4000, b"abc" * 3333 + b"ab"]:
        sa = sa_ref.suffix_array(t)
        assert sa_ref.check(t, sa) == (sa_ref.OK, sa_ref.NONE)
        assert sa_ref.check(t, sa.view(np.uint32)) == (sa_ref.OK, sa_ref.NONE) and sa_ref.verdict(t, sa) is None


@pytest.mark.parametrize("t", [b"abracadabra", b"aaaaaaaaaa", b"ab" * 30, oracle.synth_text(5, 2500), oracle.synth_rand(6, 2049), b"a" * 4100, bytes(range(256)) * 9],
                         ids=["abracadabra", "a10", "ab30", "text2500", "rand2049", "a4100", "bytes2304"])
def test_check_on_every_planted_defect(t):
    """Every defect of sa_ref.mutations: the vectorised check and the loops agree, and a defect is found."""
    sa = sa_ref.suffix_array(t)
    seen = set()
    for name, bad in sa_ref.mutations(t, sa):
        got = sa_ref.check(t, bad)
        assert got == check_by_loops(t, bad), name
        if not (bad == sa.view(np.uint32)).all():                         # (two equal neighbours swapped: b"aa..." has none, a text may)
            assert got[0] != sa_ref.OK, name
        seen.add(got[0])
    assert {sa_ref.RANGE, sa_ref.MISSING, sa_ref.ORDER} <= seen


def test_the_lower_stage_and_the_lower_row_win():
    t = oracle.synth_text(7, 3000)
    sa = sa_ref.suffix_array(t)
    got = dict((name, sa_ref.check(t, bad)) for name, bad in sa_ref.mutations(t, sa))
    assert got["order at row 2 and range at the last row"] == (sa_ref.RANGE, 2999)
    assert got["range at rows 3 and n - 2"] == (sa_ref.RANGE, 3)
    assert got["order at row 2 and a missing position"][0] == sa_ref.MISSING


def test_search_on_small_texts():
    t = b"abracadabra"
    sa = sa_ref.suffix_array(t)
    assert list(sa) == [10, 7, 0, 3, 5, 8, 1, 4, 6, 9, 2]
    assert sa_ref.search(t, sa, b"abra") == (2, 1) and sa_ref.search(t, sa, b"a") == (5, 0) and sa_ref.search(t, sa, b"") == (11, 0)
    assert sa_ref.search(t, sa, b"abrac") == (1, 2) and sa_ref.search(t, sa, b"zz") == (0, 11) and sa_ref.search(t, sa, b"ab0") == (0, 1)
    assert sa_ref.search(t, sa, b"rab") == (0, 10)                        # "ra" (row 9) is a prefix of it: it sorts in front and is no match
    for p in (b"abra", b"bra", b"cad", b"a", b"ra"):
        count, left = sa_ref.search(t, sa, p)
        assert sorted(int(s) for s in sa[left:left + count]) == [i for i in range(len(t)) if t.startswith(p, i)]


@pytest.mark.parametrize("gen,seed,n", [("synth_text", 3, 1 << 16), ("synth_rand", 4, 30000)])
def test_the_bwt_of_the_reference_array_is_the_oracles(gen, seed, n):
    """Ties the new reference to the reference project's own build: divbwt read off the array == oracle.divbwt."""
    t = getattr(oracle, gen)(seed, n)
    assert sa_ref.bwt_of(t, sa_ref.suffix_array(t)) == oracle.divbwt(t)
    for s in (b"banana", b"a", b"ab" * 50, b"\x00\x01\x00"):
        assert sa_ref.bwt_of(s, sa_ref.suffix_array(s)) == oracle.divbwt(s)
