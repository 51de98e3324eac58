"""CPU stepping of the two-component gadget kernel (tests/emu/emu_gadget2.cpp: polydot_gadget2_kernel stepped thread by
thread with the kernel's own headers: one forward transform per term, two products, two sums, two inverses) against the
stepping of the one-component kernel on the matching slices of the prepared operand, against the oracle's products of the
Python-decomposed digits, and the new entry point's argument list (csrc/api_checks.h: check_gadget_multidot), without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import P64, p64
from test_dot_emu import sum_mod
from test_gadget_emu import MODES, POLICIES, EmuGadget, decompose_rows, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FN = "tn_poly_gadget_multidot_prepared_dev"


class EmuGadget2:
    """The entry points of tests/emu/emu_gadget2.cpp in tests/emu/_build/libemu.so."""

    def __init__(self):
        L = self.lib = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_gadget_multidot_prepared.argtypes = [u32, u64, u64, ci, P64, P64, sz, P64, sz, sz, sz, u32, u32]
        L.emu_gadget2_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, vp, sz, sz, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]

    def multidot(self, n, q, psi, a, bhat, outs, terms, w, balanced=False, canonical=False):
        """a: (batch, n); bhat: (outs * terms, n) for one shared set or (batch * outs * terms, n) -> (batch, outs, n)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.shape[0]
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (outs * terms, batch * outs * terms)
        sets = 1 if bhat.shape[0] == outs * terms else batch
        c = np.empty((batch, outs, n), dtype=np.uint64)
        rc = self.lib.emu_poly_gadget_multidot_prepared(n, q, psi, int(canonical), p64(a), p64(bhat), sets, p64(c), batch, outs, terms, w, int(balanced))
        assert rc == 0, rc
        return c

    def check(self, view, a, b, c, sets=1, batch=1, outs=2, terms=1, base_log=1, flags=0):
        """check_gadget_multidot on the plan view (n, elem_bytes, has_fused, omega_only, q) -> (status, text, goes on to a launch)."""
        return emu_library.api_check(self.lib.emu_gadget2_api_check, *view, a, b, c, sets, batch, outs, terms, base_log, flags)


@pytest.fixture(scope="module")
def gadget2():
    return EmuGadget2()


@pytest.fixture(scope="module")
def gadget():
    return EmuGadget()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def pair_rows(batch, terms, outs=2):
    """Rows of a case's b for a set per output row: b[(r + o + 2 * j) % 5] is term j of component o of row r -> (batch, outs, terms)."""
    return np.array([[[(r + o + 2 * j) % 5 for j in range(terms)] for o in range(outs)] for r in range(batch)])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepped_pair_matches_the_one_component_stepping_and_the_oracle(gadget2, gadget, prep, oracle, case, canonical):
    """Batch 2, every (terms, w) of gadget_pairs, one shared set and one set per row, both digit modes: each component of the
    stepped pair equals the stepping of the one-component kernel on its slice of the prepared operand and the sum mod q of the
    oracle's products of the Python-decomposed digit rows; outs = 1 equals the existing stepping."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    row_pairs = ([0, 3], [1, 4], [2, 3], [0, 4])
    for (terms, w), rows in zip(gadget_pairs(q), row_pairs):
        a2 = a[rows]
        for shared in (True, False):
            idx = pair_rows(2, terms)                                   # (2, outs, terms) rows of b
            if shared:
                idx[1] = idx[0]
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            for balanced in MODES:
                where = (case, canonical, terms, w, shared, balanced)
                c = gadget2.multidot(n, q, psi, a2, bh, 2, terms, w, balanced, canonical)
                assert c.shape == (2, 2, n)
                digits = decompose_rows(a2, q, w, terms, balanced)
                for o in range(2):
                    bo = bhat[idx[0, o]] if shared else bhat[idx[:, o].ravel()]
                    one = gadget.poly_gadget_dot_prepared(n, q, psi, a2, bo, terms, w, balanced, canonical)
                    assert np.array_equal(c[:, o], one), where + (o,)
                    ref = sum_mod(oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(2, terms, n), q)
                    assert np.array_equal(c[:, o], ref), where + (o,)
                    c1 = gadget2.multidot(n, q, psi, a2, bo, 1, terms, w, balanced, canonical)
                    assert np.array_equal(c1[:, 0], one), where + (o,)


# ---- the argument list -------------------------------------------------------------------------
N, WORD, Q, W = 4, 4, 7681, 4                               # the smallest plan: rows of 16 bytes; 2^W < Q
ROW = N * WORD
FUSED, GENERAL, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (0, 0, 0, 0, 0)
A, B, C = 1 << 20, 1 << 30, 1 << 40
BATCH, OUTS, TERMS = 5, 2, 2
T_ROWS = FN + ": batch * outs * terms too large for one call (max 2^31 - 1 digit rows)"
T_OVERLAP = FN + ": output must not alias or overlap an input"
T_FUSED = FN + ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_SETS = FN + ": bhat_sets must be 1 (one set of operands for every row) or batch"

# (id, view, a, bhat, c, keywords, status, text or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, B, C, {}, OK, None, True),
    ("shared-ok", FUSED, A, B, C, dict(sets=1), OK, None, True),
    ("one-component-ok", FUSED, A, B, C, dict(outs=1), OK, None, True),
    ("balanced-ok", FUSED, A, B, C, dict(flags=1), OK, None, True),
    ("outs-0", FUSED, A, B, C, dict(outs=0), EINVAL, FN + ": outs must be at least 1", False),
    ("outs-3", FUSED, A, B, C, dict(outs=3), EUNSUPPORTED, FN + ": more than 2 output components are not supported", False),
    ("rows-2^31", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 29, outs=2, terms=2, base_log=1), EINVAL, T_ROWS, False),
    ("rows-2^31-one-term", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 30, outs=2, terms=1), EINVAL, T_ROWS, False),
    ("rows-2^31-minus-2", FUSED, A, 1 << 50, 1 << 58, dict(sets=1, batch=2 ** 30 - 1, outs=2, terms=1), OK, None, True),
    ("rows-batch-2^63", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 63, outs=2, terms=1), EINVAL, T_ROWS, False),
    ("c-over-last-row-of-a", FUSED, A, B, A + (BATCH - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-last-row-is-first-of-a", FUSED, A, B, A - (BATCH * OUTS - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-before-a", FUSED, A, B, A - BATCH * OUTS * ROW, {}, OK, None, True),
    ("c-just-past-a", FUSED, A, B, A + BATCH * ROW, {}, OK, None, True),
    ("c-over-first-row-of-the-set", FUSED, A, B, B - (BATCH * OUTS - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-the-set", FUSED, A, B, B + (OUTS * TERMS - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-past-the-set", FUSED, A, B, B + OUTS * TERMS * ROW, dict(sets=1), OK, None, True),
    ("c-over-last-row-of-the-sets", FUSED, A, B, B + (BATCH * OUTS * TERMS - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-the-sets", FUSED, A, B, B + BATCH * OUTS * TERMS * ROW, {}, OK, None, True),
    ("sets-2", FUSED, A, B, C, dict(sets=2), EINVAL, T_SETS, False),
    # each fault the gadget list refuses
    ("null-plan", NULL, A, B, C, {}, EINVAL, FN + ": plan is NULL", False),
    ("general-plan", GENERAL, A, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("terms-0", FUSED, A, B, C, dict(terms=0), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2", FUSED, A, B, C, dict(flags=2), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0", FUSED, A, B, C, dict(base_log=0), EINVAL, FN + ": need 1 <= base_log and 2^base_log < q", False),
    ("base-log-k", FUSED, A, B, C, dict(base_log=13), EINVAL, FN + ": need 1 <= base_log and 2^base_log < q", False),
    ("shift-64", FUSED, A, B, C, dict(terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("null-a", FUSED, None, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-bhat", FUSED, A, None, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-c", FUSED, A, B, None, {}, EINVAL, FN + ": NULL buffer", False),
    ("batch0-null", FUSED, None, None, None, dict(batch=0, sets=1), OK, None, False),
    # two faults: the existing list's order (plan, kernels, terms, flags, base_log, shift, rows, batch 0, buffers, sets, overlap)
    ("general-plan-terms-0", GENERAL, A, B, C, dict(terms=0), EUNSUPPORTED, T_FUSED, False),
    ("general-plan-null-a", GENERAL, None, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("terms-0-flag-2", FUSED, A, B, C, dict(terms=0, flags=2), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2-base-log-0", FUSED, A, B, C, dict(flags=2, base_log=0), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0-null-a", FUSED, None, B, C, dict(base_log=0), EINVAL, FN + ": need 1 <= base_log and 2^base_log < q", False),
    ("batch0-sets-2", FUSED, A, B, C, dict(batch=0, sets=2), OK, None, False),
    ("null-a-sets-2", FUSED, None, B, C, dict(sets=2), EINVAL, FN + ": NULL buffer", False),
    ("sets-2-c-is-a", FUSED, A, B, A, dict(sets=2), EINVAL, T_SETS, False),
    # the component count stands behind the plan's checks and before the gadget list's
    ("general-plan-outs-0", GENERAL, A, B, C, dict(outs=0), EUNSUPPORTED, T_FUSED, False),
    ("outs-3-terms-0", FUSED, A, B, C, dict(outs=3, terms=0), EUNSUPPORTED, FN + ": more than 2 output components are not supported", False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(gadget2, row):
    _, view, a, b, c, kw, status, text, launches = row
    full = dict(sets=BATCH, batch=BATCH, outs=OUTS, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    st, got, goes_on = gadget2.check(view, a, b, c, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got


def test_one_component_has_the_gadget_calls_answers(gadget2):
    """outs == 1: status and launch of every row of the gadget call's own table (tests/api_cases.py), texts but for the name."""
    import api_cases
    lib = emu_library.load()
    n, word, q = 256, 4, 8380417
    seen = 0
    for case in api_cases.cases(5, 2, q.bit_length()):
        if case.entry != "tn_poly_gadget_dot_prepared_dev":
            continue
        st, text, launches = api_cases.emu_case(lib, case, n, word, q)
        view = {api_cases.FUSED: (n, word, 1, 0, q), api_cases.GENERAL: (n, word, 0, 0, q), api_cases.OMEGA: (n, word, 0, 1, q),
                api_cases.NULL: (0, 0, 0, 0, 0)}[case.plan]
        g = case.args
        a, b, out = (api_cases.address(g[x], 1 << 32, n * word) for x in ("a", "b", "out"))
        st2, text2, launches2 = gadget2.check(view, a, b, out, g["sets"], g["batch"], 1, g["terms"], g["base_log"], g["flags"])
        assert (st2, launches2) == (st, launches), case.id
        assert text2 == text.replace("tn_poly_gadget_dot_prepared_dev", FN).replace("batch * terms", "batch * outs * terms"), case.id
        seen += 1
    assert seen > 30
