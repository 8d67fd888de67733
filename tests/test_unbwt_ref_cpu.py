"""CPU: the plain reference of the GPU decoder's back end (tests/unbwt_ref.py) against the oracle and against itself, and the rank
arrays tests/test_gpu_unbwt.py sends to the GPU against the fill kernels' precondition -- so that a failure of the GPU test can only
be the kernels'."""
import numpy as np
import pytest

import oracle
import unbwt_cases as cases
import unbwt_ref as ref
from conftest import edge_inputs


def some_inputs():
    rs = np.random.RandomState(11)
    out = list(edge_inputs())
    out += [("rand-%d" % n, rs.randint(0, 256, n).astype(np.uint8).tobytes()) for n in (5, 1000, 8193)]
    out += [("rand4-%d" % n, rs.choice([3, 7, 200, 255], n).astype(np.uint8).tobytes()) for n in (97, 20001)]
    out += [("periodic-7x300", bytes(rs.randint(0, 256, 7).astype(np.uint8)) * 300),
            ("periodic-257x40", bytes(rs.randint(0, 4, 257).astype(np.uint8)) * 40),
            ("halves-5000", oracle.synth_text(3, 5000) * 2),
            ("constant-8193", b"\x00" * 8193)]
    return out


INPUTS = some_inputs()


@pytest.mark.parametrize("name,data", INPUTS, ids=[n for n, _ in INPUTS])
def test_planes_then_access_gives_the_bytes_back(name, data):
    bwt, _ = oracle.bwt_stage(data)
    for b in (bwt, np.frombuffer(data, dtype=np.uint8)):          # (any bytes have planes, a BWT or not)
        bits, zeros, R_full, words, rankw = ref.planes_of(b)
        assert np.array_equal(ref.access(bits, zeros, R_full), b)
        assert np.array_equal(bits, oracle.plane_bits(b))         # the reference's own level order
        n, W = len(b), ref.plane_words(len(b))
        assert words.shape == rankw.shape == (8, W)
        for p in range(8):
            for w in range(W):                                    # the packed layout, word by word
                lo = 32 * w
                want = sum(int(bits[p][i]) << (i - lo) for i in range(lo, min(lo + 32, n)))
                assert words[p][w] == want
                assert rankw[p][w] == (int(bits[p][:lo].sum()) if lo <= n else 0)
            if W * n > 40000:
                break                                             # (one level of the long ones)


@pytest.mark.parametrize("name,data", INPUTS, ids=[n for n, _ in INPUTS])
def test_inverse_of_the_oracles_bwt_stage_is_the_input(name, data):
    bwt, off = oracle.bwt_stage(data)
    text, lc = ref.inverse(bwt, off)
    assert text is not None and text.tobytes() == data
    assert len(data) % lc == 0
    slow, lc_slow = ref.inverse_slow(bwt, off)
    assert lc_slow == lc and np.array_equal(slow, text)
    for o in (0, 1, len(data) - 1):
        t, _ = ref.inverse(bwt, o)
        assert np.array_equal(t, np.roll(text, o - off))


def test_cycle_lengths_and_refusals():
    for data, lc in ((b"a" * 64, 1), (b"ab" * 500, 2), (b"abc" * 33, 3), (oracle.synth_text(2, 5000) * 7, 5000), (b"abracadabra", 11)):
        bwt, off = oracle.bwt_stage(data)
        assert ref.inverse(bwt, off)[1] == lc
    text, lc = ref.inverse(np.frombuffer(b"abababab", dtype=np.uint8), 0)      # no BWT of anything, but row 0 is a cycle of its own
    assert lc == 1 and text.tobytes() == b"a" * 8
    bad = np.frombuffer(b"bbaab", dtype=np.uint8)                 # rows 0 -> 2 -> 0: a cycle of 2 in 5 rows
    assert ref.inverse(bad, 0) == (None, 2) == ref.inverse_slow(bad, 0)


def test_seam_reference_against_the_oracle():
    rs = np.random.RandomState(3)
    for t in [b"a", b"ab", b"banana", b"ab" * 9, oracle.synth_text(4, 8191), bytes(rs.randint(0, 3, 500).astype(np.uint8))]:
        u, p = oracle.divbwt(t)
        assert ref.seam_inverse(np.frombuffer(u, dtype=np.uint8), p).tobytes() == t == oracle.inverse_bwt(u, p)
    assert ref.seam_inverse(np.frombuffer(b"abababab", dtype=np.uint8), 1) is None      # several LF cycles


def test_walker_plan():
    assert [ref.walker_shift(r) for r in (1, 8191, 8192, 16383, 16384, (1 << 20) - 1, 1 << 20, 1 << 27, (1 << 27) + 255, (1 << 27) + 256, 1 << 28)] == \
        [0, 0, 1, 1, 2, 7, 8, 8, 8, 9, 9]
    assert ref.walkers(8191) == 8191 and ref.walkers(8192) == 4096 and ref.walkers(8193) == 4097


def test_sparse_ranks_keep_every_gap_constant():
    rs = np.random.RandomState(5)
    b = rs.randint(0, 256, 3000).astype(np.uint8)
    bits, zeros, R_full, _, _ = ref.planes_of(b)
    assert ref.gaps_constant(R_full)
    R = ref.sparse_ranks(R_full, bits)
    assert ref.gaps_constant(R) and (R == ref.K_UNKNOWN).any()
    assert np.all((R == ref.K_UNKNOWN) | (R == R_full))
    R2 = ref.sparse_ranks(R_full, bits, keep=np.array([5, 64, 96, 3000]))
    assert ref.gaps_constant(R2) and np.all(R2[:, [5, 64, 96]] == R_full[:, [5, 64, 96]])
    # ... and gaps_constant does notice: a bit change forgotten, a rank that decreases, an end unknown
    p = 0
    i = int(np.flatnonzero(bits[p][1:] != bits[p][:-1])[3]) + 1
    for mutate in (lambda R: R.__setitem__((p, i), ref.K_UNKNOWN), lambda R: R.__setitem__((p, 3000), 0),
                   lambda R: R.__setitem__((p, 0), ref.K_UNKNOWN)):
        Rm = R.copy()
        mutate(Rm)
        assert not ref.gaps_constant(Rm)


@pytest.mark.parametrize("n", cases.FILL_SIZES)
def test_every_rank_array_of_the_gpu_test_meets_the_precondition(n):
    count = 0
    for case in cases.fill_cases(n):
        assert case.R.shape == (8, n + 1) and case.R.dtype == np.uint32
        assert ref.gaps_constant(case.R), case.name
        assert np.all((case.R == ref.K_UNKNOWN) | (case.R == case.R_full)), case.name
        count += 1
    assert count >= 9


def test_edge_cases_of_the_gpu_test_meet_the_precondition_and_sit_where_they_say():
    for case in cases.edge_fill_cases():
        assert ref.gaps_constant(case.R), case.name
    last, first = cases.only_boundary_case(8191), cases.only_boundary_case(8192)
    for case, at in ((last, 8191), (first, 8192)):
        assert list(np.flatnonzero(case.R[0] != ref.K_UNKNOWN)) == [0, at, case.n]     # the only interior boundary of level 0
    assert 8191 // ref.FG_CHUNK == 0 and 8192 // ref.FG_CHUNK == 1
    for case in cases.refused_fill_cases():
        assert not ref.gaps_constant(case.R), case.name
