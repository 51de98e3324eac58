"""CPU stepping of the external-product kernel (tests/emu/emu_extprod.cpp: polydot_extprod_kernel stepped thread by
thread with the kernel's own headers: two sums over ins * terms terms, one forward transform per term, two inverses) against
the stepping of the one-component dot kernel on the concatenated Python-decomposed digits, against the oracle's products of
those digits, and the new entry point's argument list (csrc/api_checks.h: check_external_product), without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import P64, p64
from test_dot_emu import EmuDot, sum_mod
from test_gadget2_emu import EmuGadget2
from test_gadget_emu import MODES, POLICIES, decompose_rows, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FN = "tn_poly_external_product_prepared_dev"
INS = (2, 3)


class EmuExtprod:
    """The entry points of tests/emu/emu_extprod.cpp in tests/emu/_build/libemu.so."""

    def __init__(self):
        L = self.lib = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_external_product_prepared.argtypes = [u32, u64, u64, ci, P64, P64, sz, P64, sz, sz, sz, u32, u32]
        L.emu_extprod_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, vp, sz, sz, sz, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]

    def external_product(self, n, q, psi, a, bhat, terms, w, balanced=False, canonical=False):
        """a: (batch, ins, n); bhat: (2 * ins * terms, n) for one shared set or (batch * 2 * ins * terms, n) -> (batch, 2, n)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch, ins = a.shape[0], a.shape[1]
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (2 * ins * terms, batch * 2 * ins * terms)
        sets = 1 if bhat.shape[0] == 2 * ins * terms else batch
        c = np.empty((batch, 2, n), dtype=np.uint64)
        rc = self.lib.emu_poly_external_product_prepared(n, q, psi, int(canonical), p64(a), p64(bhat), sets, p64(c), batch, ins, terms, w, int(balanced))
        assert rc == 0, rc
        return c

    def check(self, view, a, b, c, sets=1, batch=1, ins=2, outs=2, terms=1, base_log=1, flags=0):
        """check_external_product on the plan view (n, elem_bytes, has_fused, omega_only, q) -> (status, text, goes on to a launch)."""
        return emu_library.api_check(self.lib.emu_extprod_api_check, *view, a, b, c, sets, batch, ins, outs, terms, base_log, flags)


@pytest.fixture(scope="module")
def extprod():
    return EmuExtprod()


@pytest.fixture(scope="module")
def gadget2():
    return EmuGadget2()


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def ext_rows(batch, ins, terms, outs=2):
    """Rows of a case's b for a set per output row: b[(r + o + 2 * i + 3 * j) % 5] is term j of input i of component o of row r
    -> (batch, outs, ins, terms)."""
    return np.array([[[[(r + o + 2 * i + 3 * j) % 5 for j in range(terms)] for i in range(ins)] for o in range(outs)] for r in range(batch)])


def input_rows(batch, ins, first=0):
    """Rows of a case's a that input polynomial i of output row r takes: the case's five rows in turn, so that every launch of two
    rows or more reads the all-(q - 1) row and unreduced full-width rows -> (batch, ins)."""
    return (first + np.arange(batch * ins).reshape(batch, ins)) % 5


def digit_rows(a, q, w, terms, balanced):
    """a (batch, ins, n) -> (batch, ins * terms, n): the Python decomposition of a viewed as batch * ins rows, which is the layout
    the dot product takes ([batch * ins][terms][n] = [batch][ins * terms][n]); carries start at 0 for every row of that view."""
    batch, ins, n = a.shape
    return decompose_rows(a.reshape(batch * ins, n), q, w, terms, balanced).reshape(batch, ins * terms, n)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepped_external_product_matches_the_dot_stepping_and_the_oracle(extprod, dot, prep, oracle, case, canonical):
    """Batch 2, ins 2 and 3, every (terms, w) of gadget_pairs, one shared set and one set per row, both digit modes: each
    component of the stepped result equals the stepping of the one-component dot kernel on the concatenated Python-decomposed
    digits and the sum mod q of the oracle's products of those digits."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    first = 0
    for ins in INS:
        for terms, w in gadget_pairs(q):
            a2 = a[input_rows(2, ins, first)]                            # (2, ins, n)
            first += 1
            for shared in (True, False):
                idx = ext_rows(2, ins, terms)                            # (2, outs, ins, terms) rows of b
                if shared:
                    idx[1] = idx[0]
                bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
                for balanced in MODES:
                    where = (case, canonical, ins, terms, w, shared, balanced)
                    c = extprod.external_product(n, q, psi, a2, bh, terms, w, balanced, canonical)
                    assert c.shape == (2, 2, n)
                    digits = digit_rows(a2, q, w, terms, balanced)
                    for o in range(2):
                        bo = bhat[idx[0, o].ravel()] if shared else bhat[idx[:, o].ravel()]
                        one = dot.poly_dot_prepared(n, q, psi, digits, bo, canonical)
                        assert np.array_equal(c[:, o], one), where + (o,)
                        prods = oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(2, ins * terms, n)
                        assert np.array_equal(c[:, o], sum_mod(prods, q)), where + (o,)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_one_input_is_the_pair_kernels_stepping(extprod, gadget2, prep, case, canonical):
    """ins = 1: the flow of the new kernel equals the stepping of the pair kernel, which is what the entry point runs then."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    terms, w = gadget_pairs(q)[1]
    a2 = a[[2, 3]]
    for shared in (True, False):
        idx = ext_rows(2, 1, terms)
        bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
        for balanced in MODES:
            c = extprod.external_product(n, q, psi, a2[:, None, :], bh, terms, w, balanced, canonical)
            assert np.array_equal(c, gadget2.multidot(n, q, psi, a2, bh, 2, terms, w, balanced, canonical)), (case, canonical, shared, balanced)


def test_carries_do_not_run_from_one_polynomial_into_the_next(extprod, prep):
    """Balanced digits whose last carry is dropped: input 0 is all q - 1 (its top digit carries out where the digits do not cover
    q), and the result is the one of input 1 preceded by any other polynomial's digits, term by term."""
    n, q, psi, a, b = _case_data("P256")
    bhat = prep.prepare(n, q, psi, b)
    terms, w = 2, 8                                                  # 16 bits of a 23-bit q: the carry out of digit 1 is dropped
    idx = ext_rows(1, 2, terms)
    bh = bhat[idx.ravel()]
    first = extprod.external_product(n, q, psi, np.stack([a[3], a[0]])[None], bh, terms, w, True)
    other = extprod.external_product(n, q, psi, np.stack([np.zeros_like(a[3]), a[0]])[None], bh, terms, w, True)
    alone = extprod.external_product(n, q, psi, np.stack([a[3], np.zeros_like(a[0])])[None], bh, terms, w, True)
    assert np.array_equal(first, (other + alone) % np.uint64(q))


# ---- the argument list -------------------------------------------------------------------------
N, WORD, Q, W = 4, 4, 7681, 4                               # the smallest plan: rows of 16 bytes; 2^W < Q
ROW = N * WORD
FUSED, GENERAL, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (0, 0, 0, 0, 0)
A, B, C = 1 << 20, 1 << 30, 1 << 40
BATCH, INS_, OUTS, TERMS = 5, 3, 2, 2
T_ROWS = FN + ": batch * outs * ins * terms too large for one call (max 2^31 - 1 digit rows)"
T_OVERLAP = FN + ": output must not alias or overlap an input"
T_FUSED = FN + ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_SETS = FN + ": bhat_sets must be 1 (one set of operands for every row) or batch"
T_INS = FN + ": ins must be at least 1"
T_OUTS3 = FN + ": more than 2 output components are not supported"
T_INS_OUTS = FN + (": 2 or more input polynomials into 1 output component are not supported (tn_gadget_decompose_dev, then "
                   "tn_poly_dot_prepared_dev)")
T_BASE = FN + ": need 1 <= base_log and 2^base_log < q"
SET = OUTS * INS_ * TERMS                                    # rows of one set

# (id, view, a, bhat, c, keywords, status, text or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, B, C, {}, OK, None, True),
    ("shared-ok", FUSED, A, B, C, dict(sets=1), OK, None, True),
    ("two-inputs-ok", FUSED, A, B, C, dict(ins=2), OK, None, True),
    ("one-input-ok", FUSED, A, B, C, dict(ins=1), OK, None, True),
    ("one-input-one-component-ok", FUSED, A, B, C, dict(ins=1, outs=1), OK, None, True),
    ("balanced-ok", FUSED, A, B, C, dict(flags=1), OK, None, True),
    # one row per fault, in the order of the list
    ("null-plan", NULL, A, B, C, {}, EINVAL, FN + ": plan is NULL", False),
    ("general-plan", GENERAL, A, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("ins-0", FUSED, A, B, C, dict(ins=0), EINVAL, T_INS, False),
    ("outs-0", FUSED, A, B, C, dict(outs=0), EINVAL, FN + ": outs must be at least 1", False),
    ("outs-3", FUSED, A, B, C, dict(outs=3), EUNSUPPORTED, T_OUTS3, False),
    ("two-inputs-one-component", FUSED, A, B, C, dict(ins=2, outs=1), EUNSUPPORTED, T_INS_OUTS, False),
    ("three-inputs-one-component", FUSED, A, B, C, dict(outs=1), EUNSUPPORTED, T_INS_OUTS, False),
    ("terms-0", FUSED, A, B, C, dict(terms=0), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2", FUSED, A, B, C, dict(flags=2), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0", FUSED, A, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("base-log-k", FUSED, A, B, C, dict(base_log=13), EINVAL, T_BASE, False),
    ("shift-64", FUSED, A, B, C, dict(terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-2^31", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 28, ins=2, outs=2, terms=2, base_log=1), EINVAL, T_ROWS, False),
    ("rows-2^31-one-term", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 29, ins=2, outs=2, terms=1), EINVAL, T_ROWS, False),
    ("rows-2^31-minus-4", FUSED, A, 1 << 50, 1 << 58, dict(sets=1, batch=2 ** 29 - 1, ins=2, outs=2, terms=1), OK, None, True),
    ("rows-batch-2^63", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 63, ins=2, outs=2, terms=1), EINVAL, T_ROWS, False),
    ("rows-ins-2^62", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2, ins=2 ** 62, outs=2, terms=1), EINVAL, T_ROWS, False),
    ("rows-ins-2^63-batch-2", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2, ins=2 ** 63, outs=2, terms=2), EINVAL, T_ROWS, False),
    ("rows-ins-2^31-batch-2^31", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 31, ins=2 ** 31, outs=2, terms=2), EINVAL, T_ROWS, False),
    ("batch0-null", FUSED, None, None, None, dict(batch=0, sets=1), OK, None, False),
    ("null-a", FUSED, None, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-bhat", FUSED, A, None, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-c", FUSED, A, B, None, {}, EINVAL, FN + ": NULL buffer", False),
    ("sets-2", FUSED, A, B, C, dict(sets=2), EINVAL, T_SETS, False),
    # overlap by byte range: c's batch * outs rows against a's batch * ins rows ...
    ("c-is-a", FUSED, A, B, A, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-a", FUSED, A, B, A + (BATCH * INS_ - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-last-row-is-first-of-a", FUSED, A, B, A - (BATCH * OUTS - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-last-byte-is-first-of-a", FUSED, A, B, A - BATCH * OUTS * ROW + 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-before-a", FUSED, A, B, A - BATCH * OUTS * ROW, {}, OK, None, True),
    ("c-over-last-byte-of-a", FUSED, A, B, A + BATCH * INS_ * ROW - 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-a", FUSED, A, B, A + BATCH * INS_ * ROW, {}, OK, None, True),
    ("c-past-batch-rows-of-a-two-inputs", FUSED, A, B, A + BATCH * ROW, dict(ins=2), EINVAL, T_OVERLAP, False),
    # ... against a shared set's outs * ins * terms rows ...
    ("c-over-first-row-of-the-set", FUSED, A, B, B - (BATCH * OUTS - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-before-the-set", FUSED, A, B, B - BATCH * OUTS * ROW, dict(sets=1), OK, None, True),
    ("c-over-last-row-of-the-set", FUSED, A, B, B + (SET - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-past-the-set", FUSED, A, B, B + SET * ROW, dict(sets=1), OK, None, True),
    # ... and against the batch sets of a launch with a set per row
    ("c-over-first-row-of-the-sets", FUSED, A, B, B - (BATCH * OUTS - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-before-the-sets", FUSED, A, B, B - BATCH * OUTS * ROW, {}, OK, None, True),
    ("c-past-the-first-set-of-the-sets", FUSED, A, B, B + SET * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-the-sets", FUSED, A, B, B + (BATCH * SET - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-the-sets", FUSED, A, B, B + BATCH * SET * ROW, {}, OK, None, True),
    # two faults: the order (plan, kernels, ins, outs, ins with outs, terms, flags, base_log, shift, rows, batch 0, buffers, sets, overlap)
    ("null-plan-ins-0", NULL, A, B, C, dict(ins=0), EINVAL, FN + ": plan is NULL", False),
    ("general-plan-ins-0", GENERAL, A, B, C, dict(ins=0), EUNSUPPORTED, T_FUSED, False),
    ("general-plan-null-a", GENERAL, None, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("ins-0-outs-0", FUSED, A, B, C, dict(ins=0, outs=0), EINVAL, T_INS, False),
    ("ins-0-outs-3", FUSED, A, B, C, dict(ins=0, outs=3), EINVAL, T_INS, False),
    ("outs-0-two-inputs", FUSED, A, B, C, dict(ins=2, outs=0), EINVAL, FN + ": outs must be at least 1", False),
    ("outs-3-terms-0", FUSED, A, B, C, dict(outs=3, terms=0), EUNSUPPORTED, T_OUTS3, False),
    ("one-component-terms-0", FUSED, A, B, C, dict(outs=1, terms=0), EUNSUPPORTED, T_INS_OUTS, False),
    ("one-component-batch-0", FUSED, None, None, None, dict(outs=1, batch=0, sets=1), EUNSUPPORTED, T_INS_OUTS, False),
    ("terms-0-flag-2", FUSED, A, B, C, dict(terms=0, flags=2), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2-base-log-0", FUSED, A, B, C, dict(flags=2, base_log=0), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0-null-a", FUSED, None, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("shift-64-rows", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 31, terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-batch-0-is-no-row", FUSED, None, None, None, dict(batch=0, sets=1, ins=2 ** 40), OK, None, False),
    ("rows-null-a", FUSED, None, 4096, 4096, dict(sets=1, batch=2 ** 30, ins=2), EINVAL, T_ROWS, False),
    ("batch0-sets-2", FUSED, A, B, C, dict(batch=0, sets=2), OK, None, False),
    ("null-a-sets-2", FUSED, None, B, C, dict(sets=2), EINVAL, FN + ": NULL buffer", False),
    ("sets-2-c-is-a", FUSED, A, B, A, dict(sets=2), EINVAL, T_SETS, False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(extprod, row):
    _, view, a, b, c, kw, status, text, launches = row
    full = dict(sets=BATCH, batch=BATCH, ins=INS_, outs=OUTS, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    st, got, goes_on = extprod.check(view, a, b, c, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got


def test_one_input_has_the_multidot_calls_answers(extprod, gadget2):
    """ins == 1: status, launch and text (but for the names) of every row of the multidot call's own table."""
    import test_gadget2_emu as g2
    for row in g2.TABLE:
        _, view, a, b, c, kw, status, text, launches = row
        full = dict(sets=g2.BATCH, batch=g2.BATCH, outs=g2.OUTS, terms=g2.TERMS, base_log=g2.W, flags=0)
        full.update(kw)
        st, got, goes_on = extprod.check(view, a, b, c, ins=1, **full)
        assert (st, goes_on) == (status, launches), row[0]
        assert got == (text or "").replace(g2.FN, FN).replace("batch * outs * terms", "batch * outs * ins * terms"), row[0]
