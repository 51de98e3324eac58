"""GPU tests of the prepared, dot-product, transform-domain and gadget entry points (and the fused product beside them) at the
policy-boundary moduli of tests/policy_moduli.py (its QUICK subset): the last prime each bound schedule accepts and the first it
refuses, the word-size points from 20 to 62 bits, lazy and forced canonical plans.  Every result is compared with the oracle (and
the digit definition) first, then with the device's own equivalent calls.  The CPU stepping of the same kernels at the full table
is tests/test_policy_moduli_emu.py; nothing here needs it."""
import numpy as np
import pytest

from chosen_rows import SHAPES, chosen_rows
from policy_moduli import ENTRIES, QUICK, entry_id, psi_of, sum_terms
from test_dot_emu import term_rows
from test_gadget_emu import MODES, decompose_rows, gadget_pairs
from test_gpu_dot import device_sum
from test_prepared_emu import operand_rows

pytestmark = pytest.mark.gpu

BATCH = 5
Q60 = 1152921504606830593
# (n, q) of test_chosen_prepared_words: the 23-bit lazy boundary at n = 256, a 31-bit q (32-bit lanes, canonical: acc + x < 2q
# just fits the word), the first n = 4096 modulus that is lazy without the base case, the last that takes it, and n = 8192
CHOSEN_WORDS = [(256, 8372737), (4096, 2147377153), (4096, 1152921504576864257), (4096, 1152921504577118209), (8192, Q60)]
BC_QUICK = [(e[0], e[1]) for e in QUICK if e[3]]
SPECTRA = SHAPES + [s for s in BC_QUICK if s not in SHAPES]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


def host(plan, t):
    return plan.to_host(t).astype(np.uint64)


def check_entry(eng, plan, oracle, n, q, psi):
    """Every new entry point on one plan, batch 5, terms <= 3 (5 one-bit digits in one gadget call)."""
    import torch
    where = (n, q, plan.is_lazy)
    Q = np.uint64(q)
    a, b = operand_rows(n, q, n + q % 1000)
    da, db = plan.to_device(a), plan.to_device(b)
    diag = oracle.poly_mult(a, b, q, psi)
    assert diag[4, 0] == q - 1 and not diag[4, 1:].any()                      # x^(n-1) * x = -1

    assert np.array_equal(host(plan, plan.poly_mult(da, db, variant="fused")), diag), where
    # prepare: canonical words that depend on the operand mod q only; unprepare inverts it both ways
    pa, pb = plan.prepare(da), plan.prepare(db)
    for x, px in ((a, pa), (b, pb)):
        assert int(host(plan, px.tensor).max()) < q, where
        assert torch.equal(px.tensor, plan.prepare(x % Q).tensor), where
        back = plan.unprepare(px)
        assert np.array_equal(host(plan, back), x % Q), where
        assert torch.equal(plan.prepare(back).tensor, px.tensor), where
    # prepared product: one prepared row per row, and one shared row
    assert np.array_equal(host(plan, plan.poly_mult_prepared(da, pb)), diag), where
    one = eng.PreparedOperand(plan, pb.tensor[:1], 1)
    assert np.array_equal(host(plan, plan.poly_mult_prepared(da, one)), oracle.poly_mult(a, np.repeat(b[:1], BATCH, axis=0), q, psi)), where
    assert torch.equal(plan.poly_dot_hat(pa, pb), plan.poly_mult(da, db, variant="fused")), where
    # dot products: the oracle, then prepared dot == dot of prepared rows == summed fused products
    for terms in (2, 3):
        flat = term_rows(BATCH, terms).ravel()
        for shared in (False, True):
            at = (where, terms, shared)
            bidx = np.tile(np.arange(terms), BATCH) if shared else flat
            a3 = plan.to_device(a[flat]).reshape(BATCH, terms, n)
            pb_t = plan.prepare(b[:terms] if shared else b[flat])
            pa_t = plan.prepare(a[flat])
            want = sum_terms(oracle.poly_mult(a[flat], b[bidx], q, psi).reshape(BATCH, terms, n), q)
            dc = plan.poly_dot_prepared(a3, pb_t)
            assert np.array_equal(host(plan, dc), want), at
            assert torch.equal(plan.poly_dot_hat(pa_t, pb_t, terms), dc), at
            assert torch.equal(device_sum(plan, a3, plan.to_device(b[bidx]).reshape(BATCH, terms, n)), dc), at
            kept = plan.poly_dot_hat(pa_t, pb_t, terms, keep_prepared=True)
            assert kept.rows == BATCH and torch.equal(kept.tensor, plan.prepare(dc).tensor), at
            assert torch.equal(plan.unprepare(kept), dc), at
    # gadget: the digits against the definition, the fused call against the oracle's products of them and decompose + dot
    for terms, w in gadget_pairs(q):
        for shared in (True, False):
            bidx = np.tile(np.arange(terms), BATCH) if shared else term_rows(BATCH, terms).ravel()
            pb_t = plan.prepare(b[bidx[:terms]] if shared else b[bidx])
            for balanced in MODES:
                at = (where, terms, w, shared, balanced)
                want_digits = decompose_rows(a, q, w, terms, balanced)
                digits = plan.gadget_decompose(da, terms, w, balanced)
                assert np.array_equal(host(plan, digits.reshape(-1, n)).reshape(BATCH, terms, n), want_digits), at
                want = sum_terms(oracle.poly_mult(want_digits.reshape(-1, n), b[bidx], q, psi).reshape(BATCH, terms, n), q)
                c = plan.poly_gadget_dot_prepared(da, pb_t, terms, w, balanced)
                assert np.array_equal(host(plan, c), want), at
                assert torch.equal(c, plan.poly_dot_prepared(digits, pb_t)), at


@pytest.mark.parametrize("entry", QUICK, ids=[entry_id(e) for e in QUICK])
def test_entry_points_at_policy_boundary_moduli(eng, oracle, entry):
    """One case per modulus (each names its (n, q) and stays short): the plan the library picks, and for a lazy one the forced
    canonical plan too."""
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    for flags in ((0, eng.PLAN_FORCE_CANONICAL) if lazy else (0,)):
        plan = eng.Plan(n, q, psi, 0, flags)
        try:
            assert plan.has_fused and plan.is_lazy == (lazy and flags == 0), (n, q, flags)
            assert plan.elem_bytes == (4 if q < 2 ** 31 else 8)
            check_entry(eng, plan, oracle, n, q, psi)
        finally:
            plan.close()


def chosen_words(n, q, rng):
    """Prepared rows the test chooses (any words below q are valid prepared rows): a_rows / b_rows (batch, terms, n), terms = 4.
    Row 0 multiplies q - 1 by 1 in every term, so every accumulate adds q - 1 to a running sum (q - 1, q - 2, ...) and wraps; row 1
    adds (q - 1)^2 = 1 four times; the others mix 0, 1, q - 1, the alternating row and random words."""
    M, ONE, Z = (np.full(n, v, dtype=np.uint64) for v in (q - 1, 1, 0))
    ALT = np.tile(np.array([q - 1, 1], dtype=np.uint64), n // 2)
    R = rng.integers(0, q, (4, n), dtype=np.uint64)
    a_rows = np.array([[M, M, M, M], [M, M, M, M], [ALT, M, ONE, R[0]], [R[0], R[1], R[2], R[3]], [Z, M, ALT, M]])
    b_rows = np.array([[ONE, ONE, ONE, ONE], [M, M, M, M], [ALT, ALT, M, R[1]], [R[3], R[2], R[1], R[0]], [R[0], ONE, ALT, ONE]])
    return a_rows, b_rows


@pytest.mark.parametrize("n,q", CHOSEN_WORDS, ids=[f"n{n}_q{q}" for n, q in CHOSEN_WORDS])
def test_chosen_prepared_words(eng, oracle, n, q):
    """tn_poly_dot_hat_dev on prepared words picked by the test, terms = 4, per-row and shared second operand.  Without the base
    case the prepared output is the word-wise sum of products mod q (Python integers) and the coefficients are its unprepare();
    with the base case the coefficients are the oracle's summed products of the unprepared rows."""
    import torch
    psi = psi_of(n, q)
    lazy, bc = next(e[2:] for e in ENTRIES if (e[0], e[1]) == (n, q))
    plan = eng.get_plan(n, q, psi)
    assert plan.is_lazy == lazy
    terms = 4
    a_rows, b_rows = chosen_words(n, q, np.random.default_rng(q % 1000))
    batch = a_rows.shape[0]
    assert int(a_rows.max()) < q and int(b_rows.max()) < q
    pa = eng.PreparedOperand(plan, plan.to_device(a_rows.reshape(-1, n)), batch * terms)
    for shared in (False, True):
        bw = np.repeat(b_rows[2:3], batch, axis=0) if shared else b_rows                  # shared set: ALT, ALT, q - 1, random
        pb = eng.PreparedOperand(plan, plan.to_device(bw[0] if shared else bw.reshape(-1, n)), terms if shared else batch * terms)
        c = plan.poly_dot_hat(pa, pb, terms)
        kept = plan.poly_dot_hat(pa, pb, terms, keep_prepared=True)
        assert int(host(plan, kept.tensor).max()) < q and int(host(plan, c).max()) < q
        if not bc:
            want = ((a_rows.astype(object) * bw.astype(object)).sum(axis=1) % q).astype(np.uint64)
            if not shared:
                assert (want[0] == (4 * (q - 1)) % q).all() and (want[1] == 4).all()
            assert np.array_equal(host(plan, kept.tensor), want), (n, q, shared)
            assert torch.equal(c, plan.unprepare(eng.PreparedOperand(plan, plan.to_device(want), batch))), (n, q, shared)
        else:
            ua, ub = host(plan, plan.unprepare(pa)), host(plan, plan.unprepare(pb))
            if shared:
                ub = np.tile(ub, (batch, 1))
            want = sum_terms(oracle.poly_mult(ua, ub, q, psi).reshape(batch, terms, n), q)
            assert np.array_equal(host(plan, c), want), (n, q, shared)
        assert torch.equal(plan.unprepare(kept), c), (n, q, shared)
        assert torch.equal(plan.prepare(c).tensor, kept.tensor), (n, q, shared)


@pytest.mark.parametrize("n,q", SPECTRA, ids=[f"n{n}_q{q}" for n, q in SPECTRA])
def test_chosen_spectra_through_the_prepared_kernels(eng, oracle, n, q):
    """GPU twin of test_policy_moduli_emu.py's test of the same name: the chosen-spectrum rows, their unreduced twins and the
    fold-boundary rows of tests/chosen_rows.py through the prepared product, the product of prepared rows and a 2-term dot product,
    both policies; without the base case a prepared row is a permutation of the chosen spectrum."""
    psi = psi_of(n, q)
    cr = chosen_rows(oracle, n, q)
    m, rows = cr.nspec, cr.a.shape[0]
    bc = (n, q) in BC_QUICK
    for flags in (0, eng.PLAN_FORCE_CANONICAL):
        plan = eng.get_plan(n, q, psi, 0, flags)
        assert plan.has_fused and plan.is_lazy == (flags == 0)
        where = (n, q, flags)
        da = plan.to_device(np.array(cr.a))
        pa, pb = plan.prepare(da), plan.prepare(np.array(cr.b))
        got = host(plan, plan.poly_mult_prepared(da, pb))
        assert np.array_equal(got, cr.ref), (where, np.nonzero((got != cr.ref).any(axis=1))[0].tolist())
        got = host(plan, plan.poly_dot_hat(pa, pb))
        assert np.array_equal(got, cr.ref), (where, np.nonzero((got != cr.ref).any(axis=1))[0].tolist())
        if not (bc and flags == 0):                      # (a canonical-policy plan never runs the base case)
            ahat, bhat = host(plan, pa.tensor), host(plan, pb.tensor)
            for r in range(2 * m):
                assert np.array_equal(np.sort(ahat[r]), np.sort(cr.Sa[r % m])), (where, r)
                assert np.array_equal(np.sort(bhat[r]), np.sort(cr.Sb[r % m])), (where, r)
        first = np.arange(rows - 1)
        idx = np.stack([first, first + 1], axis=1)       # output row r: a[r] b[r] + a[r+1] b[r+1]
        want = sum_terms(np.stack([cr.ref[:-1], cr.ref[1:]], axis=1), q)
        got = host(plan, plan.poly_dot_prepared(plan.to_device(cr.a[idx.ravel()]).reshape(rows - 1, 2, n), plan.prepare(cr.b[idx.ravel()])))
        assert np.array_equal(got, want), (where, np.nonzero((got != want).any(axis=1))[0].tolist())
