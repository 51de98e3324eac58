"""CPU stepping of the gadget dot-product kernel (tests/emu/emu_gadget.cpp: polydot_gadget_kernel stepped thread by thread with
the kernel's own headers and its canonicalise-and-digit functions) against the definition of include/tinyntt.h written out in
Python with big integers, the stepping of the prepared dot product on those digits, and the oracle, without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import PARAMS, P64, p64
from test_dot_emu import EmuDot, sum_mod, term_rows
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

POLICIES = pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])
MODES = (False, True)                      # unsigned, balanced


class EmuGadget:
    """The gadget entry points of tests/emu/_build/libemu.so (tests/emu/emu_gadget.cpp)."""

    def __init__(self):
        L = self.lib = emu_library.load()
        u32, u64, sz, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_gadget_dot_prepared.argtypes = [u32, u64, u64, ci, P64, P64, sz, P64, sz, sz, u32, u32]
        L.emu_gadget_digits.argtypes = [u32, u64, u64, ci, P64, P64, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.POINTER(ci)]

    def poly_gadget_dot_prepared(self, n, q, psi, a, bhat, terms, w, balanced=False, canonical=False):
        """a: (batch, n); bhat: (terms, n) for one shared set or (batch * terms, n)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.shape[0]
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (terms, batch * terms)
        sets = 1 if bhat.shape[0] == terms else batch
        c = np.empty((batch, n), dtype=np.uint64)
        rc = self.lib.emu_poly_gadget_dot_prepared(n, q, psi, int(canonical), p64(a), p64(bhat), sets, p64(c), batch, terms, w, int(balanced))
        assert rc == 0, rc
        return c

    def digits(self, n, q, psi, words, terms, w, balanced=False, canonical=False):
        """gadget_digit(gadget_canon(word), j) of the plan's lane width and policy -> ((count, terms) digits, lane bytes, lazy)."""
        x = np.ascontiguousarray(words, dtype=np.uint64)
        out = np.empty((x.size, terms), dtype=np.uint64)
        lane, lazy = ctypes.c_int(), ctypes.c_int()
        rc = self.lib.emu_gadget_digits(n, q, psi, int(canonical), p64(x), p64(out), x.size, terms, w, int(balanced), ctypes.byref(lane), ctypes.byref(lazy))
        assert rc == 0, rc
        return out, lane.value, bool(lazy.value)


@pytest.fixture(scope="module")
def gadget():
    return EmuGadget()


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def digits_of_word(x, q, w, terms, balanced):
    """The definition with Python integers: (signed digits d_j, the carry out of the last digit)."""
    xh, B = int(x) % q, 1 << w
    out, carry = [], 0
    for j in range(terms):
        u = (xh >> (j * w)) & (B - 1)
        if not balanced:
            out.append(u)
            continue
        t = u + carry
        if t >= B // 2:
            out.append(t - B); carry = 1
        else:
            out.append(t); carry = 0
    return out, carry


def decompose_rows(a, q, w, terms, balanced):
    """The definition on whole rows: a (batch, n) of any words -> (batch, terms, n) canonical residues (uint64).  The same steps
    as digits_of_word on numpy words (every quantity stays below 2^63); test_row_decomposition_is_the_word_definition ties the two."""
    assert (terms - 1) * w < 64 and (1 << w) < q
    xh = np.asarray(a, dtype=np.uint64) % np.uint64(q)
    B = np.uint64(1 << w)
    out = np.empty((xh.shape[0], terms, xh.shape[1]), dtype=np.uint64)
    carry = np.zeros(xh.shape, dtype=np.uint64)
    for j in range(terms):
        t = ((xh >> np.uint64(j * w)) & (B - np.uint64(1))) + carry
        neg = (t >= B // np.uint64(2)) if balanced else np.zeros(xh.shape, dtype=bool)
        out[:, j] = np.where(neg, (np.uint64(q) - (B - t)) % np.uint64(q), t)
        carry = neg.astype(np.uint64)
    return out


def gadget_pairs(q):
    """The (terms, w) pairs of the kernel tests: digits that cover q in 2 and in 3 terms, 5 one-bit digits, 2 digits of k - 1 bits."""
    k = q.bit_length()
    return [(2, -(-k // 2)), (3, -(-k // 3)), (5, 1), (2, k - 1)]


def contract_words(q, w, lane_bits, rng, count=1000):
    """The words of the digit contract: the edges of the digits, of q and of the lane, then `count` random words of the lane."""
    k, B = q.bit_length(), 1 << w
    full = (1 << lane_bits) - 1
    T = (k - 1) // w                               # digits that fit below 2^(k-1) <= q: the word is its own residue
    all_top = (1 << (T * w)) - 1                   # every unsigned digit B - 1: the carry runs through all of them
    half_run = sum((B // 2 - 1) << (j * w) for j in range(T)) + 1      # digits B/2 - 1 with a lowest digit of B/2
    assert all_top < q and half_run < q
    words = [0, 1, B // 2 - 1, B // 2, B - 1, B, q - 1, q, q + 1, 2 * q - 1, 1 << k, full, all_top, half_run]
    assert all(0 <= x <= full for x in words)
    return words + [int(v) for v in rng.integers(0, full, count, dtype=np.uint64, endpoint=True)]


def check_digit_contract(gadget, n, q, psi, canonical, lazy, count=1000):
    """gadget_canon + gadget_digit of the plan (n, q, psi) against the big-integer definition on contract_words, both modes, and
    the two sums the definition implies.  lazy: the policy the plan must report.  (tests/test_policy_moduli_emu.py runs this at
    every modulus of tests/policy_moduli.py.)"""
    k = q.bit_length()
    lane_bits = 32 if q < 2 ** 31 else 64
    rng = np.random.default_rng(q % 1000 + canonical)
    for w in sorted({1, 2, 7, -(-k // 2), k - 1}):
        B = 1 << w
        words = contract_words(q, w, lane_bits, rng, count)
        cover = -(-k // w)                         # terms * w >= k
        for terms in sorted({1, 3, (k - 1) // w, cover}):
            if terms < 1 or (terms - 1) * w >= 64:
                continue
            for balanced in MODES:
                out, lane, got_lazy = gadget.digits(n, q, psi, words, terms, w, balanced, canonical)
                assert lane * 8 == lane_bits and got_lazy == lazy
                for x, got in zip(words, out):
                    d, carry = digits_of_word(x, q, w, terms, balanced)
                    assert [int(v) for v in got] == [v % q for v in d], (n, q, canonical, w, terms, balanced, x)
                    assert all(-(B // 2) <= v < B // 2 for v in d) if balanced else all(0 <= v < B for v in d)
                    total = sum(v << (j * w) for j, v in enumerate(d))
                    if balanced:
                        assert total == (x % q) % B ** terms - carry * B ** terms
                    elif terms * w >= k:
                        assert total == x % q


@pytest.mark.parametrize("case", ["P4096_60", "P1024"])
@POLICIES
def test_digit_contract(gadget, case, canonical):
    """gadget_canon + gadget_digit against the big-integer definition for ANY word of the lane (64-bit and 32-bit lanes, lazy
    and canonical policy), both modes, and the two sums the definition implies."""
    n, q, psi = PARAMS[case]
    k = q.bit_length()
    check_digit_contract(gadget, n, q, psi, canonical, not canonical)
    # the carry does run through every digit of those two words
    w = 7
    T = (k - 1) // w
    d, carry = digits_of_word((1 << (T * w)) - 1, q, w, T, True)
    assert d == [-1] + [0] * (T - 1) and carry == 1
    d, carry = digits_of_word(sum((64 - 1) << (j * w) for j in range(T)) + 1, q, w, T, True)
    assert d == [-64] * T and carry == 1


def test_row_decomposition_is_the_word_definition():
    """decompose_rows (numpy words; what the kernel tests compare with) is digits_of_word on every word."""
    for case in ("P4096_60", "P1024"):
        _, q, _ = PARAMS[case]
        rng = np.random.default_rng(q % 97)
        full = 2 ** 64 - 1 if q > 2 ** 32 else 2 ** 32 - 1
        a = rng.integers(0, full, (2, 64), dtype=np.uint64, endpoint=True)
        a[0, :4] = (0, q - 1, q, full)
        for terms, w in gadget_pairs(q) + [(1, 7)]:
            for balanced in MODES:
                rows = decompose_rows(a, q, w, terms, balanced)
                for r in range(2):
                    for i in range(64):
                        d, _ = digits_of_word(a[r, i], q, w, terms, balanced)
                        assert [int(v) for v in rows[r, :, i]] == [v % q for v in d]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepped_kernel_matches_the_dot_product_of_the_digits(gadget, dot, prep, oracle, case, canonical):
    """Batch 2, both modes, one shared set and one set per row, four (terms, w) pairs: the stepped kernel equals the stepped
    prepared dot product on the Python-decomposed digits and the sum mod q of the oracle's products of those digit rows.  The
    case's rows hold full-width unreduced words, the all-(q - 1) row and a monomial; every pair of them is used."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    row_pairs = ([0, 3], [1, 4], [2, 3], [0, 4])
    for (terms, w), rows in zip(gadget_pairs(q), row_pairs):
        a2 = a[rows]
        for shared in (True, False):
            bidx = np.tile(np.arange(terms), 2) if shared else term_rows(2, terms).ravel()
            bh = bhat[:terms] if shared else bhat[bidx]
            for balanced in MODES:
                digits = decompose_rows(a2, q, w, terms, balanced)
                c = gadget.poly_gadget_dot_prepared(n, q, psi, a2, bh, terms, w, balanced, canonical)
                where = (case, canonical, terms, w, shared, balanced)
                assert np.array_equal(c, dot.poly_dot_prepared(n, q, psi, digits, bh, canonical)), where
                ref = sum_mod(oracle.poly_mult(digits.reshape(-1, n), b[bidx], q, psi).reshape(2, terms, n), q)
                assert np.array_equal(c, ref), where


@pytest.mark.parametrize("case", ["P4096_60", "P1024"])
@POLICIES
def test_one_term_is_one_digit_and_the_prepared_product(gadget, prep, case, canonical):
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b[:2], canonical)
    for balanced in MODES:
        digits = decompose_rows(a[:2], q, 7, 1, balanced)
        c = gadget.poly_gadget_dot_prepared(n, q, psi, a[:2], bhat, 1, 7, balanced, canonical)
        assert np.array_equal(c, prep.poly_mult_prepared(n, q, psi, digits[:, 0], bhat, canonical))


def test_stepping_refuses_what_the_calls_refuse(gadget):
    n, q, psi, a, b = _case_data("P1024")
    k = q.bit_length()
    a2 = np.ascontiguousarray(a[:2])
    bh = np.ascontiguousarray(b[:4])                   # never read: every call below is refused first
    c = np.empty((2, n), dtype=np.uint64)
    L = gadget.lib

    def run(sets, terms, w, flags, batch=2):
        return L.emu_poly_gadget_dot_prepared(n, q, psi, 0, p64(a2), p64(bh), sets, p64(c), batch, terms, w, flags)

    assert run(1, 0, 7, 0) != 0                        # terms == 0
    assert run(1, 2, 0, 0) != 0                        # base_log == 0
    assert run(1, 2, k, 0) != 0                        # 2^base_log >= q
    assert run(1, 2, 64, 0) != 0
    assert run(1, 11, 7, 0) != 0                       # (terms - 1) * base_log = 70
    assert run(1, 65, 1, 0) != 0                       # (terms - 1) * base_log = 64
    assert run(1, 2, 7, 2) != 0                        # unknown flag bit
    assert run(3, 2, 7, 0) != 0                        # bhat_sets neither 1 nor batch
    assert L.emu_poly_gadget_dot_prepared(n, q, psi + 1, 0, p64(a2), p64(bh), 1, p64(c), 2, 2, 7, 0) != 0     # not a primitive 2n-th root
    out = np.empty((2, 3), dtype=np.uint64)
    words = np.array([1, 2], dtype=np.uint64)
    for terms, w, flags in ((0, 7, 0), (3, 0, 0), (3, k, 0), (11, 7, 0), (3, 7, 4)):
        assert L.emu_gadget_digits(n, q, psi, 0, p64(words), p64(out), 2, terms, w, flags, None, None) != 0
    # the largest shifts that are allowed do run: 64 one-bit digits, and a shift past the width of a 32-bit lane gives zeros
    d, lane, _ = gadget.digits(n, q, psi, [q - 1, 2 ** 32 - 1], 64, 1)
    assert lane == 4
    for x, got in zip((q - 1, 2 ** 32 - 1), d):
        assert [int(v) for v in got] == digits_of_word(x, q, 1, 64, False)[0]
        assert not got[k:].any()
