"""CPU stepping of the fused product and of the prepared, dot-product, transform-domain and gadget kernels at the moduli of
tests/policy_moduli.py: the last prime each bound schedule accepts and the first it refuses, per size and word length, the
word-size points (20 to 62 bits) and the reference's moduli, under the lazy policy where a plan takes it and under the forced
canonical policy always.  Expected values come from the oracle and from the big-integer digit definition; the table's flags are
checked against plan_tables.h first.  No GPU.  (GPU twin: tests/test_gpu_policy_moduli.py.)"""
import ctypes

import numpy as np
import pytest

from chosen_rows import SHAPES, chosen_rows
from conftest import P64, ntt_prime_below, p64
from policy_moduli import BC_ENTRIES, ENTRIES, PAIRS, QUICK, entry_id, lane_bits, psi_of, sum_terms
from test_dot_emu import EmuDot, dot_reference, term_rows
from test_gadget_emu import MODES, EmuGadget, check_digit_contract, decompose_rows, gadget_pairs
from test_hat_emu import EmuHat
from test_prepared_emu import EmuPrepared, operand_rows

# every entry under the forced canonical policy, the lazy ones under the lazy policy too
RUNS = [(e, canonical) for e in ENTRIES for canonical in ((False, True) if e[2] else (True,))]
RUN_IDS = [entry_id(e) + ("-canonical" if canonical else "-lazy") for e, canonical in RUNS]
# chosen spectra: every fused shape of chosen_rows.py (none of them but (4096, Q60) takes the base case) and every base-case entry
SPECTRA = SHAPES + [(e[0], e[1]) for e in BC_ENTRIES if (e[0], e[1]) not in SHAPES]


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def hat():
    return EmuHat()


@pytest.fixture(scope="module")
def gadget():
    return EmuGadget()


@pytest.fixture(scope="module")
def flags(emu):
    L = emu.lib
    L.bc_enabled.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
    L.bc_polymul.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, P64, P64, P64, ctypes.c_size_t, ctypes.c_int]

    def get(n, q):
        psi = psi_of(n, q)
        return L.emu_is_lazy(n, q, psi), L.bc_enabled(n, q, psi)
    return get


def test_table_flags_and_boundary_pairs(flags):
    """Every entry's flags are what plan_tables.h decides for it, and every boundary pair is a boundary: two consecutive NTT
    primes, the first with the flag and the second without.  A change to a bound schedule that moves a boundary fails here."""
    for n, q, lazy, bc in ENTRIES:
        assert (q - 1) % (2 * n) == 0 and q < 2 ** 62
        assert flags(n, q) == (int(lazy), int(bc)), (n, q)
    table = {(n, q): (lazy, bc) for n, q, lazy, bc in ENTRIES}
    assert len(table) == len(ENTRIES)
    for n, flag, first, second in PAIRS:
        assert ntt_prime_below(first, n) == second, (n, flag, first, second)
        assert first.bit_length() == second.bit_length()
        which = {"lazy": 0, "bc": 1}[flag]
        assert flags(n, first)[which] == 1 and flags(n, second)[which] == 0, (n, flag, first, second)
        assert table[(n, first)][which] and not table[(n, second)][which], (n, flag, first, second)


def test_table_covers_both_policies_lane_widths_and_the_base_case():
    for n in (256, 4096, 8192):
        for bits in (32, 64):
            for lazy in (True, False):
                assert any(e[0] == n and lane_bits(e[1]) == bits and e[2] == lazy for e in ENTRIES), (n, bits, lazy)
        for k in (23, 26, 50, 55, 59, 60):
            pair = [p for p in PAIRS if p[0] == n and p[1] == "lazy" and p[2].bit_length() == k]
            assert len(pair) == (0 if (n, k) == (8192, 23) else 1), (n, k)
        for k in (31, 32, 61, 62):                       # the word-size edges, never lazy
            assert any(e[0] == n and e[1].bit_length() == k and not e[2] for e in ENTRIES), (n, k)
    assert not any(e[0] == 8192 and e[1] < 2 ** 23 and e[2] for e in ENTRIES)      # no 13-bit-c NTT prime fits below 2^23 there
    assert all(e[0] == 4096 and e[2] and lane_bits(e[1]) == 64 for e in BC_ENTRIES)
    assert len({e[1].bit_length() for e in BC_ENTRIES}) >= 4
    assert len([e for e in ENTRIES if e[0] == 4096 and lane_bits(e[1]) == 64 and e[2] and not e[3]]) >= 2
    assert set(QUICK) <= set(ENTRIES) and {e for e in ENTRIES if e[0] == 4096 and e[3]} <= set(QUICK)
    for n, flag, first, second in PAIRS:
        if n == 4096 or (flag == "lazy" and first.bit_length() in (26, 60)):
            assert {(n, first), (n, second)} <= {(e[0], e[1]) for e in QUICK}


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_kernels_match_the_oracle(emu, prep, dot, hat, gadget, oracle, flags, entry, canonical):
    """The rows of test_prepared_emu.operand_rows (unreduced random words, all q - 1, x^(n-1) * x) through every stepped kernel."""
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    where = (n, q, canonical)
    Q = np.uint64(q)
    a, b = operand_rows(n, q, n + q % 1000)
    pairs = sorted({(i, i) for i in range(5)} | {(i, k) for i in range(5) for k in range(3)})
    ref = oracle.poly_mult(a[[i for i, _ in pairs]], b[[k for _, k in pairs]], q, psi)
    prods = {pair: ref[t] for t, pair in enumerate(pairs)}
    diag = np.stack([prods[(i, i)] for i in range(5)])
    assert diag[4, 0] == q - 1 and not diag[4, 1:].any()                      # x^(n-1) * x = -1

    # the three-transform product, and the base-case product where the plan takes it
    assert np.array_equal(emu.fused(n, q, psi, a, b, canonical=canonical), diag), where
    if bc and not canonical:
        c = np.empty_like(a)
        assert emu.lib.bc_polymul(n, q, psi, p64(a), p64(b), p64(c), 5, 0) == 0
        assert np.array_equal(c, diag), where

    # prepare: canonical words that depend on the operand mod q only
    ahat, bhat = prep.prepare(n, q, psi, a, canonical), prep.prepare(n, q, psi, b, canonical)
    assert int(ahat.max()) < q and int(bhat.max()) < q, where
    assert np.array_equal(bhat, prep.prepare(n, q, psi, b % Q, canonical)), where

    # prepared product, one prepared row per row and one shared row
    assert np.array_equal(prep.poly_mult_prepared(n, q, psi, a, bhat, canonical), diag), where
    shared = np.stack([prods[(i, 0)] for i in range(5)])
    assert np.array_equal(prep.poly_mult_prepared(n, q, psi, a, bhat[:1], canonical), shared), where

    # dot products of un-prepared and of prepared rows; a result kept prepared is prepare() of the coefficients
    for terms in (2, 3):
        idx = term_rows(2, terms)
        flat = idx.ravel()
        for one_set in (False, True):
            bh = bhat[:terms] if one_set else bhat[flat]
            want = dot_reference(prods, q, idx, one_set)
            assert np.array_equal(dot.poly_dot_prepared(n, q, psi, a[idx], bh, canonical), want), (where, terms, one_set)
            assert np.array_equal(hat.poly_dot_hat(n, q, psi, ahat[flat], bh, terms, canonical), want), (where, terms, one_set)
            kept = hat.poly_dot_hat(n, q, psi, ahat[flat], bh, terms, canonical, keep_prepared=True)
            assert np.array_equal(kept, prep.prepare(n, q, psi, want, canonical)), (where, terms, one_set)

    # unprepare inverts prepare, both ways
    for x, xhat in ((a, ahat), (b, bhat)):
        back = hat.unprepare(n, q, psi, xhat, canonical)
        assert np.array_equal(back, x % Q), where
        assert np.array_equal(prep.prepare(n, q, psi, back, canonical), xhat), where

    # gadget product against the oracle's products of the digit rows of the definition
    for (terms, w), rows in zip(gadget_pairs(q), ([0, 3], [1, 4], [2, 3], [0, 4])):
        a2 = a[rows]
        for one_set in (True, False):
            bidx = np.tile(np.arange(terms), 2) if one_set else term_rows(2, terms).ravel()
            bh = bhat[:terms] if one_set else bhat[bidx]
            for balanced in MODES:
                digits = decompose_rows(a2, q, w, terms, balanced)
                want = sum_terms(oracle.poly_mult(digits.reshape(-1, n), b[bidx], q, psi).reshape(2, terms, n), q)
                got = gadget.poly_gadget_dot_prepared(n, q, psi, a2, bh, terms, w, balanced, canonical)
                assert np.array_equal(got, want), (where, terms, w, one_set, balanced)


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_digit_contract_at_every_modulus(gadget, entry, canonical):
    """test_gadget_emu.py's digit contract (0, B/2, B - 1, q - 1, q, 2q - 1, 2^k, the full word, carries through every digit, random
    words) for every (k, c) of the table: one fold of any word must land below 2q, which is nearest to failing at the boundaries.
    100 random words per digit width instead of 1000: the edges are what differs from modulus to modulus."""
    n, q, lazy, bc = entry
    check_digit_contract(gadget, n, q, psi_of(n, q), canonical, lazy and not canonical, count=100)


@pytest.mark.parametrize("n,q", SPECTRA, ids=[f"n{n}_q{q}" for n, q in SPECTRA])
def test_chosen_spectra_through_the_prepared_kernels(prep, dot, hat, oracle, flags, n, q):
    """Rows whose spectrum was chosen (tests/chosen_rows.py: entries 0, 1, 2, (q-1)/2, (q+1)/2, q-2, q-1), their unreduced twins
    and the fold-boundary rows through the pointwise step and base case of the prepared, dot-product and transform-domain kernels,
    both policies.  Without the base case a prepared row is a permutation of the chosen spectrum itself."""
    psi = psi_of(n, q)
    lazy, bc = flags(n, q)
    assert lazy == 1 and bc == ((n, q) in [(e[0], e[1]) for e in BC_ENTRIES])
    cr = chosen_rows(oracle, n, q)
    m, rows = cr.nspec, cr.a.shape[0]
    for canonical in (False, True):
        where = (n, q, canonical)
        ahat, bhat = prep.prepare(n, q, psi, cr.a, canonical), prep.prepare(n, q, psi, cr.b, canonical)
        got = prep.poly_mult_prepared(n, q, psi, cr.a, bhat, canonical)
        assert np.array_equal(got, cr.ref), (where, np.nonzero((got != cr.ref).any(axis=1))[0].tolist())
        got = hat.poly_dot_hat(n, q, psi, ahat, bhat, 1, canonical)
        assert np.array_equal(got, cr.ref), (where, np.nonzero((got != cr.ref).any(axis=1))[0].tolist())
        if not (bc and not canonical):                   # (a canonical-policy plan never runs the base case)
            for r in range(2 * m):
                assert np.array_equal(np.sort(ahat[r]), np.sort(cr.Sa[r % m])), (where, r)
                assert np.array_equal(np.sort(bhat[r]), np.sort(cr.Sb[r % m])), (where, r)
        first = np.arange(rows - 1)
        idx = np.stack([first, first + 1], axis=1)       # output row r: a[r] b[r] + a[r+1] b[r+1]
        want = sum_terms(np.stack([cr.ref[:-1], cr.ref[1:]], axis=1), q)
        got = dot.poly_dot_prepared(n, q, psi, cr.a[idx], bhat[idx.ravel()], canonical)
        assert np.array_equal(got, want), (where, np.nonzero((got != want).any(axis=1))[0].tolist())
