"""CPU: the one-shot compression chooses the depth h of K1's first sort, and the sort's key may carry the rotation's
preceding byte.

Two claims are checked here, on the CPU:
  * for every depth the policy may choose, the enumeration's trace on the order sorted h symbols deep is the true trace
    through round 8 h - 1 (the check of test_partial_order_cpu.py, at those depths);
  * a stable LSD radix sort of (key << 8 | T[p - 1]) on the bits from 8 up, in the digits the wide sorter takes, leaves the keys
    in the order of `partial_bwt` whatever the low byte holds, so the sorted keys' low bytes are the provisional BWT.
"""
import numpy as np
import pytest

import oracle
import test_partial_order_cpu as po

DEPTHS = [("text-1M", lambda: oracle.synth_text(12, 1 << 20), h) for h in (7, 8, 9, 10)] + [("rand-64K", lambda: oracle.synth_rand(13, 64 << 10), 7)]


@pytest.mark.parametrize("name,make,h", DEPTHS, ids=["%s-h%d" % (c[0], c[2]) for c in DEPTHS])
def test_trace_is_true_through_the_cap_at_every_depth_of_the_policy(name, make, h):
    po.test_early_rounds_do_not_need_the_finished_order(name, make, h)


def symbol_keys(t, h):
    """(key of the first h symbols of every rotation, bits per symbol): the alphabet compacted in byte order, as K1 does."""
    n = len(t)
    present = np.zeros(256, dtype=bool)
    present[t] = True
    code = np.cumsum(present) - 1
    sigma = int(present.sum())
    bits = max(1, int(np.ceil(np.log2(sigma)))) if sigma > 1 else 1
    assert h * bits + 8 <= 64
    pos = np.arange(n, dtype=np.int64)
    key = np.zeros(n, dtype=np.uint64)
    for j in range(h):
        key = (key << np.uint64(bits)) | code[t[(pos + j) % n]].astype(np.uint64)
    return key, bits


def lsd_sort(key, val, first_bit, bits, max_digit=9):
    """The wide sorter's passes: balanced digits of at most `max_digit` bits on key bits [first_bit, first_bit + bits), stable."""
    npass = (bits + max_digit - 1) // max_digit
    done = 0
    for p in range(npass):
        left, pleft = bits - done, npass - p
        nb = (left + pleft - 1) // pleft
        digit = (key >> np.uint64(first_bit + done)) & np.uint64((1 << nb) - 1)
        order = np.argsort(digit, kind="stable")
        key, val = key[order], val[order]
        done += nb
    assert done == bits
    return key, val


CARRY = {
    "text-70001": (lambda: oracle.synth_text(16, 70001), (7, 8, 9, 10, 11)),      # n odd, no multiple of a tile or of four
    "rand-4099": (lambda: oracle.synth_rand(17, 4099), (7,)),                    # 8-bit symbols: 56 + 8 bits, the whole key
    "ab": (lambda: b"ab" * 4097, (1, 7, 16)),
    "three": (lambda: b"cab", (1, 7)),                                           # h > n
    "one-byte": (lambda: b"q" * 501, (7,)),
}
CARRY_CASES = [(name, h) for name, (_, hs) in CARRY.items() for h in hs]


@pytest.mark.parametrize("name,h", CARRY_CASES, ids=["%s-h%d" % c for c in CARRY_CASES])
def test_carried_byte_is_the_provisional_bwt(name, h):
    data = bytes(CARRY[name][0]())
    t = np.frombuffer(data, dtype=np.uint8)
    n = len(t)
    key, bits = symbol_keys(t, h)
    prev = t[(np.arange(n) - 1) % n]
    assert prev[0] == t[n - 1]                                                  # p = 0 takes the text's last byte
    pos = np.arange(n, dtype=np.int64)
    want = po.partial_bwt(data, h)

    carried = (key << np.uint64(8)) | prev.astype(np.uint64)
    sk, sv = lsd_sort(carried, pos, 8, h * bits)
    assert np.array_equal((sk & np.uint64(0xFF)).astype(np.uint8), want)
    assert np.array_equal(t[(sv - 1) % n], want)                                # the gather from the same order agrees
    assert np.array_equal(sk >> np.uint64(8), key[sv])

    # the plain key on bits from 0 up gives the same order, and so does any other low byte
    _, sv0 = lsd_sort(key, pos, 0, h * bits)
    assert np.array_equal(sv0, sv)
    junk = np.random.RandomState(5).randint(0, 256, n).astype(np.uint64)
    _, sv1 = lsd_sort((key << np.uint64(8)) | junk, pos, 8, h * bits)
    assert np.array_equal(sv1, sv)

    # group heads: keys compared above the byte (the mask k1_finish gives the heads kernel) are the plain keys' heads
    lo = (sk & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    hi = (sk >> np.uint64(32)).astype(np.uint32)
    heads = np.r_[True, (hi[1:] != hi[:-1]) | (((lo[1:] ^ lo[:-1]) & np.uint32(0xFFFFFF00)) != 0)]
    plain = key[sv]
    assert np.array_equal(heads, np.r_[True, plain[1:] != plain[:-1]])
