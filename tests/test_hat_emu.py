"""CPU stepping of the transform-domain kernels (tests/emu/emu_hat.cpp: unprepare_fused_kernel and polydot_hat_kernel stepped
thread by thread with the kernels' own headers, product and accumulate functions and prepared-order index map) against the
oracle and against the stepping of the prepare and prepared dot-product kernels, without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import P64, p64
from test_dot_emu import EmuDot, dot_reference, products, term_rows          # noqa: F401  (products: a fixture)
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

POLICIES = pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])


class EmuHat:
    """The transform-domain entry points of tests/emu/_build/libemu.so (tests/emu/emu_hat.cpp)."""

    def __init__(self):
        L = self.lib = emu_library.load()
        u32, u64, sz, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_unprepare.argtypes = [u32, u64, u64, ci, P64, P64, sz]
        L.emu_poly_dot_hat.argtypes = [u32, u64, u64, ci, P64, P64, sz, P64, sz, sz, ci]

    def unprepare(self, n, q, psi, xhat, canonical=False):
        xhat = np.atleast_2d(np.ascontiguousarray(xhat, dtype=np.uint64))
        x = np.empty_like(xhat)
        rc = self.lib.emu_unprepare(n, q, psi, int(canonical), p64(xhat), p64(x), xhat.shape[0])
        assert rc == 0, rc
        return x

    def poly_dot_hat(self, n, q, psi, ahat, bhat, terms, canonical=False, keep_prepared=False):
        """ahat: (batch * terms, n) prepared rows; bhat: (terms, n) for one shared set or (batch * terms, n)."""
        ahat = np.ascontiguousarray(ahat, dtype=np.uint64).reshape(-1, n)
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert ahat.shape[0] % terms == 0
        batch = ahat.shape[0] // terms
        assert bhat.shape[0] in (terms, batch * terms)
        sets = 1 if bhat.shape[0] == terms else batch
        out = np.empty((batch, n), dtype=np.uint64)
        rc = self.lib.emu_poly_dot_hat(n, q, psi, int(canonical), p64(ahat), p64(bhat), sets, p64(out), batch, terms, int(keep_prepared))
        assert rc == 0, rc
        return out


@pytest.fixture(scope="module")
def hat():
    return EmuHat()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def prepared_rows(prep):
    """prepare() of a case's ten rows (a's five, then b's five) per policy, computed once and left unchanged."""
    cache = {}

    def get(case, canonical):
        if (case, canonical) not in cache:
            n, q, psi, a, b = _case_data(case)
            rows = prep.prepare(n, q, psi, np.concatenate([a, b]), canonical)
            rows.setflags(write=False)
            cache[(case, canonical)] = rows[:5], rows[5:]
        return cache[(case, canonical)]
    return get


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_unprepare_inverts_prepare_both_ways(hat, prep, prepared_rows, case, canonical):
    """unprepare(prepare(x)) == x mod q on the unreduced rows of operand_rows (the all-(q - 1) row and the monomials among
    them), canonical words out; prepare(unprepare(xhat)) == xhat word for word."""
    n, q, psi, a, b = _case_data(case)
    ahat, bhat = prepared_rows(case, canonical)
    for x, xhat in ((a, ahat), (b, bhat)):
        back = hat.unprepare(n, q, psi, xhat, canonical)
        assert int(back.max()) < q
        assert np.array_equal(back, x % np.uint64(q)), (case, canonical)
        assert np.array_equal(prep.prepare(n, q, psi, back, canonical), xhat), (case, canonical)
    assert np.array_equal(hat.unprepare(n, q, psi, ahat, canonical)[3], np.full(n, q - 1, dtype=np.uint64))
    assert hat.lib.emu_unprepare(n, q, psi, int(canonical), None, p64(np.empty((1, n), dtype=np.uint64)), 1) == 3


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_dot_of_prepared_rows_matches_oracle_and_prepared_dot_stepping(hat, prep, dot, products, prepared_rows, case, canonical):
    """terms 1, 2, 3 at batch 2, the terms taken cyclically from the case's rows; one shared set of b rows and one set per output
    row.  The coefficient output equals the oracle's summed products and the stepping of polydot_prepared_kernel on the
    un-prepared a; the prepared output equals prepare() of that result, word for word."""
    n, q, psi, a, b = _case_data(case)
    prods = products(case)
    assert prods[(4, 4)][0] == q - 1 and not prods[(4, 4)][1:].any()          # x^(n-1) * x = -1
    ahat, bhat = prepared_rows(case, canonical)
    for terms in (1, 2, 3):
        idx = term_rows(2, terms)
        flat = idx.ravel()
        for shared in (False, True):
            bh = bhat[:terms] if shared else bhat[flat]
            ref = dot_reference(prods, q, idx, shared)
            c = hat.poly_dot_hat(n, q, psi, ahat[flat], bh, terms, canonical)
            assert np.array_equal(c, ref), (case, canonical, terms, shared)
            assert np.array_equal(c, dot.poly_dot_prepared(n, q, psi, a[idx], bh, canonical)), (case, canonical, terms, shared)
            chat = hat.poly_dot_hat(n, q, psi, ahat[flat], bh, terms, canonical, keep_prepared=True)
            assert np.array_equal(chat, prep.prepare(n, q, psi, ref, canonical)), (case, canonical, terms, shared)
    out = np.empty((3, n), dtype=np.uint64)
    six = np.ascontiguousarray(ahat[term_rows(3, 2).ravel()])
    assert hat.lib.emu_poly_dot_hat(n, q, psi, int(canonical), p64(six), p64(six), 2, p64(out), 3, 2, 0) == 3     # bhat_sets neither 1 nor batch
    assert hat.lib.emu_poly_dot_hat(n, q, psi, int(canonical), p64(six), p64(six), 3, p64(out), 3, 2, 2) == 3     # out_prepared neither 0 nor 1
    assert hat.lib.emu_poly_dot_hat(n, q, psi, int(canonical), p64(six), p64(six), 3, p64(out), 3, 0, 0) == 3     # terms == 0


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_prepared_rows_add_word_wise(hat, prep, prepared_rows, case, canonical):
    """(prepare(a) + prepare(b)) mod q == prepare((a + b) mod q), for the complete transform and for the base-case form; and a
    sum of two prepared results unprepares to the sum of the two coefficient results."""
    n, q, psi, a, b = _case_data(case)
    ahat, bhat = prepared_rows(case, canonical)
    Q = np.uint64(q)
    word_sum = (ahat + bhat) % Q                                              # canonical words, 2 q < 2^64
    poly_sum = (a % Q + b % Q) % Q
    assert np.array_equal(word_sum, prep.prepare(n, q, psi, poly_sum, canonical)), (case, canonical)
    assert np.array_equal(hat.unprepare(n, q, psi, word_sum, canonical), poly_sum), (case, canonical)
    c0 = hat.poly_dot_hat(n, q, psi, ahat[:4], bhat[:2], 2, canonical)
    c1 = hat.poly_dot_hat(n, q, psi, ahat[1:5], bhat[2:4], 2, canonical)
    h0 = hat.poly_dot_hat(n, q, psi, ahat[:4], bhat[:2], 2, canonical, keep_prepared=True)
    h1 = hat.poly_dot_hat(n, q, psi, ahat[1:5], bhat[2:4], 2, canonical, keep_prepared=True)
    assert np.array_equal(hat.unprepare(n, q, psi, (h0 + h1) % Q, canonical), (c0 + c1) % Q), (case, canonical)
