"""CPU stepping of the CMux rotation kernel (tests/emu/emu_cmux.cpp: polydot_cmux_kernel stepped thread by thread with the
kernel's own headers: the masked exponent, rotated-minus-own words, one forward transform per term, two inverses, the add-in)
against a numpy statement of the definition (the monomial product in numpy, the stepping of the external-product kernel, the
addition mod q), against the oracle's products of the Python-decomposed digits, against an algebraic identity that does not
pass through the project's decomposition, and the two entry points' argument lists (csrc/api_checks.h: check_monomial,
check_cmux_rotate), without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import P64, p64
from test_dot_emu import sum_mod
from test_extprod_emu import EmuExtprod, digit_rows, ext_rows, input_rows
from test_gadget_emu import MODES, POLICIES, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FN, FNM = "tn_poly_cmux_rotate_prepared_dev", "tn_monomial_mul_dev"
BATCH = 7
P32 = ctypes.POINTER(ctypes.c_uint32)


def exponents(n):
    """One exponent per row of a launch of batch 7: no rotation, one place, the last place before the wrap, the negation, one
    place past it, the last exponent below 2n and an unreduced one (2n + 3 is 3)."""
    return np.array([0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n + 3], dtype=np.uint32)


def monomial_np(a, exps, q, minus_one=False):
    """The definition of include/tinyntt.h on numpy words: a (batch, group, n) of any words, exps (batch,) of any integers ->
    rot_e(a), or (rot_e(a) - a) mod q, canonical residues (uint64; q < 2^63, so q + q fits)."""
    a = np.asarray(a, dtype=np.uint64)
    batch, group, n = a.shape
    q64 = np.uint64(q)
    out = np.empty_like(a)
    t = np.arange(n)
    for r in range(batch):
        e = int(exps[r]) % (2 * n)
        s = (t - e) % (2 * n)
        x = a[r][:, s % n] % q64
        rot = np.where(s >= n, (q64 - x) % q64, x)
        out[r] = (rot + (q64 - a[r] % q64)) % q64 if minus_one else rot
    return out


class EmuCmux:
    """The entry points of tests/emu/emu_cmux.cpp in tests/emu/_build/libemu.so."""

    def __init__(self):
        L = self.lib = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_cmux_rotate_prepared.argtypes = [u32, u64, u64, ci, P64, P32, P64, sz, P64, sz, sz, u32, u32]
        L.emu_monomial_mul.argtypes = [u32, u64, P64, P32, P64, sz, sz, u32]
        L.emu_monomial_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, vp, sz, sz, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]
        L.emu_cmux_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, vp, vp, sz, sz, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]

    def rotate(self, n, q, psi, a, exps, bhat, terms, w, balanced=False, canonical=False):
        """a: (batch, 2, n); exps: (batch,); bhat: (4 * terms, n) for one shared key or (batch * 4 * terms, n) -> (batch, 2, n)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.shape[0]
        assert a.shape[1:] == (2, n)
        e = np.ascontiguousarray(exps, dtype=np.uint32)
        assert e.shape == (batch,)
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (4 * terms, batch * 4 * terms)
        sets = 1 if bhat.shape[0] == 4 * terms else batch
        c = np.empty((batch, 2, n), dtype=np.uint64)
        rc = self.lib.emu_poly_cmux_rotate_prepared(n, q, psi, int(canonical), p64(a), e.ctypes.data_as(P32), p64(bhat), sets, p64(c), batch, terms, w,
                                                    int(balanced))
        assert rc == 0, rc
        return c

    def monomial(self, n, q, a, exps, minus_one=False):
        """a: (batch, group, n) -> (batch, group, n), plain C++ from the definition."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch, group = a.shape[:2]
        e = np.ascontiguousarray(exps, dtype=np.uint32)
        out = np.empty_like(a)
        rc = self.lib.emu_monomial_mul(n, q, p64(a), e.ctypes.data_as(P32), p64(out), batch, group, int(minus_one))
        assert rc == 0, rc
        return out

    def check(self, view, a, e, b, c, sets=1, batch=1, comps=2, terms=1, base_log=1, flags=0):
        """check_cmux_rotate on the plan view (n, elem_bytes, has_fused, omega_only, q) -> (status, text, goes on to a launch)."""
        return emu_library.api_check(self.lib.emu_cmux_api_check, *view, a, e, b, c, sets, batch, comps, terms, base_log, flags)

    def check_monomial(self, view, a, e, out, batch=1, group=1, flags=0):
        return emu_library.api_check(self.lib.emu_monomial_api_check, *view, a, e, out, batch, group, flags)


@pytest.fixture(scope="module")
def cmux():
    return EmuCmux()


@pytest.fixture(scope="module")
def extprod():
    return EmuExtprod()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def key_rows(batch, terms, shared):
    """Rows of a case's b for the key: ext_rows with two inputs ((batch, 2, 2, terms)); a shared key is row 0's for every row."""
    idx = ext_rows(batch, 2, terms)
    if shared:
        idx[1:] = idx[0]
    return idx


def definition(extprod, n, q, psi, a, exps, bh, terms, w, balanced, canonical):
    """The numpy statement: the monomial in numpy, the stepping of the external-product kernel, (a % q + .) % q."""
    m = monomial_np(a, exps, q, True)
    return m, (a % np.uint64(q) + extprod.external_product(n, q, psi, m, bh, terms, w, balanced, canonical)) % np.uint64(q)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepped_rotation_matches_the_definition_and_the_oracle(cmux, extprod, prep, oracle, case, canonical):
    """Batch 7 with a wrap, both signs and an unreduced exponent in every launch, every (terms, w) of gadget_pairs, a shared key
    and a key per row, both digit modes: the stepped result equals the numpy statement of the definition and, per component,
    a mod q plus the sum mod q of the oracle's products of the Python-decomposed digits of the numpy monomial product."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    exps = exponents(n)
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        a7 = np.ascontiguousarray(a[input_rows(BATCH, 2, first)])        # (7, 2, n)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            for balanced in MODES:
                where = (case, canonical, terms, w, shared, balanced)
                c = cmux.rotate(n, q, psi, a7, exps, bh, terms, w, balanced, canonical)
                m, ref = definition(extprod, n, q, psi, a7, exps, bh, terms, w, balanced, canonical)
                assert np.array_equal(c, ref), where
                digits = digit_rows(m, q, w, terms, balanced)
                for o in range(2):
                    prods = oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(BATCH, 2 * terms, n)
                    assert np.array_equal(c[:, o], (a7[:, o] % np.uint64(q) + sum_mod(prods, q)) % np.uint64(q)), where + (o,)


# The algebraic test: a noise-free trivial RGSW of a bit m, b[o][i][j] = m * 2^(j w) as a constant polynomial for o == i, else 0,
# with unsigned digits that cover q: the digits recompose exactly, so the step returns rot_e(a) for m = 1 and a mod q for m = 0.
TRIVIAL = {60: (3, 21), 23: (3, 8)}                  # (terms, w) per word length of q: terms * w >= bitlen(q), 2^w < q


def trivial_key(n, q, m, terms, w):
    """(4 * terms, n): [o][i][j] = m * 2^(j w) at coefficient 0 for o == i."""
    b = np.zeros((2, 2, terms, n), dtype=np.uint64)
    for o in range(2):
        for j in range(terms):
            b[o, o, j, 0] = (m << (j * w)) % q
    return b.reshape(4 * terms, n)


@pytest.mark.parametrize("case", ["P256", "P1024", "P4096_60"])
@POLICIES
def test_trivial_rgsw_of_a_bit_selects_the_rotation(cmux, prep, case, canonical):
    n, q, psi, a, _ = _case_data(case)
    terms, w = TRIVIAL[q.bit_length()]
    assert terms * w >= q.bit_length() and (1 << w) < q and (terms - 1) * w < 64
    exps = exponents(n)
    a7 = np.ascontiguousarray(a[input_rows(BATCH, 2)])
    for m in (0, 1):
        bh = prep.prepare(n, q, psi, trivial_key(n, q, m, terms, w), canonical)
        c = cmux.rotate(n, q, psi, a7, exps, bh, terms, w, False, canonical)
        want = monomial_np(a7, exps, q) if m else a7 % np.uint64(q)
        assert np.array_equal(c, want), (case, canonical, m)


@pytest.mark.parametrize("n,q", [(16, 8380417), (256, 8380417), (1024, 1152921504606830593)])
def test_monomial_product_is_the_definition(cmux, n, q):
    """emu_monomial_mul (plain C++) against the numpy statement, both flags, group 1 and 2, any words and any exponents; and the
    numpy statement itself against X^e * a by schoolbook on one row."""
    rng = np.random.default_rng(n + q % 97)
    exps = np.concatenate([exponents(n), rng.integers(0, 2 ** 32, 3, dtype=np.uint64).astype(np.uint32)])
    for group in (1, 2):
        a = rng.integers(0, 2 ** 64 - 1, (len(exps), group, n), dtype=np.uint64, endpoint=True)
        a[0, 0, :3] = (0, q, q - 1)
        for minus_one in (False, True):
            assert np.array_equal(cmux.monomial(n, q, a, exps, minus_one), monomial_np(a, exps, q, minus_one)), (group, minus_one)
    # X^e * x with Python integers
    x = [int(v) % q for v in a[1, 0]]
    for e in (1, n - 1, n, 2 * n - 1):
        want = [0] * n
        for i, v in enumerate(x):
            k = (i + e) % (2 * n)
            want[k % n] = v if k < n else (q - v) % q
        got = monomial_np(a[1:2, :1], [e], q)[0, 0]
        assert [int(v) for v in got] == want, e


# ---- the argument lists ------------------------------------------------------------------------
N, WORD, Q, W = 4, 4, 7681, 4                               # the smallest plan: rows of 16 bytes; 2^W < Q
ROW = N * WORD
FUSED, GENERAL, OMEGA, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (N, WORD, 0, 1, Q), (0, 0, 0, 0, 0)
A, B, C, E = 1 << 20, 1 << 30, 1 << 40, 1 << 44
BATCH_, COMPS, TERMS = 5, 2, 2
T_ROWS = FN + ": batch * comps * comps * terms too large for one call (max 2^31 - 1 digit rows)"
T_OVERLAP = FN + ": output must not alias or overlap an input"
T_FUSED = FN + ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_SETS = FN + ": bhat_sets must be 1 (one set of operands for every row) or batch"
T_COMPS0 = FN + ": comps must be 2"
T_COMPS = FN + ": comps other than 2 is not supported (tn_monomial_mul_dev, tn_poly_external_product_prepared_dev, then an addition)"
T_BASE = FN + ": need 1 <= base_log and 2^base_log < q"
SET = COMPS * COMPS * TERMS                                 # rows of one key

# (id, view, a, exps, bhat, c, keywords, status, text or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, E, B, C, {}, OK, None, True),
    ("shared-ok", FUSED, A, E, B, C, dict(sets=1), OK, None, True),
    ("balanced-ok", FUSED, A, E, B, C, dict(flags=1), OK, None, True),
    # one row per fault, in the order of the list
    ("null-plan", NULL, A, E, B, C, {}, EINVAL, FN + ": plan is NULL", False),
    ("general-plan", GENERAL, A, E, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("comps-0", FUSED, A, E, B, C, dict(comps=0), EINVAL, T_COMPS0, False),
    ("comps-1", FUSED, A, E, B, C, dict(comps=1), EUNSUPPORTED, T_COMPS, False),
    ("comps-3", FUSED, A, E, B, C, dict(comps=3), EUNSUPPORTED, T_COMPS, False),
    ("terms-0", FUSED, A, E, B, C, dict(terms=0), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2", FUSED, A, E, B, C, dict(flags=2), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0", FUSED, A, E, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("base-log-k", FUSED, A, E, B, C, dict(base_log=13), EINVAL, T_BASE, False),
    ("shift-64", FUSED, A, E, B, C, dict(terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-2^31", FUSED, 4096, 4096, 4096, 4096, dict(sets=1, batch=2 ** 28, terms=2, base_log=1), EINVAL, T_ROWS, False),
    ("rows-2^31-one-term", FUSED, 4096, 4096, 4096, 4096, dict(sets=1, batch=2 ** 29, terms=1), EINVAL, T_ROWS, False),
    ("rows-2^31-minus-4", FUSED, A, E, 1 << 50, 1 << 58, dict(sets=1, batch=2 ** 29 - 1, terms=1), OK, None, True),
    ("rows-batch-2^63", FUSED, 4096, 4096, 4096, 4096, dict(sets=1, batch=2 ** 63, terms=1), EINVAL, T_ROWS, False),
    ("batch0-null", FUSED, None, None, None, None, dict(batch=0, sets=1), OK, None, False),
    ("null-a", FUSED, None, E, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-exps", FUSED, A, None, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-bhat", FUSED, A, E, None, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-c", FUSED, A, E, B, None, {}, EINVAL, FN + ": NULL buffer", False),
    ("sets-2", FUSED, A, E, B, C, dict(sets=2), EINVAL, T_SETS, False),
    # overlap by byte range: c's batch * 2 rows against a's batch * 2 rows ...
    ("c-is-a", FUSED, A, E, B, A, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-a", FUSED, A, E, B, A + (BATCH_ * COMPS - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-last-byte-is-first-of-a", FUSED, A, E, B, A - BATCH_ * COMPS * ROW + 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-before-a", FUSED, A, E, B, A - BATCH_ * COMPS * ROW, {}, OK, None, True),
    ("c-over-last-byte-of-a", FUSED, A, E, B, A + BATCH_ * COMPS * ROW - 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-a", FUSED, A, E, B, A + BATCH_ * COMPS * ROW, {}, OK, None, True),
    # ... against a shared key's 4 * terms rows ...
    ("c-over-first-row-of-the-key", FUSED, A, E, B, B - (BATCH_ * COMPS - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-before-the-key", FUSED, A, E, B, B - BATCH_ * COMPS * ROW, dict(sets=1), OK, None, True),
    ("c-over-last-row-of-the-key", FUSED, A, E, B, B + (SET - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-past-the-key", FUSED, A, E, B, B + SET * ROW, dict(sets=1), OK, None, True),
    # ... and against the batch keys of a launch with a key per row
    ("c-past-the-first-key-of-the-keys", FUSED, A, E, B, B + SET * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-the-keys", FUSED, A, E, B, B + (BATCH_ * SET - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-the-keys", FUSED, A, E, B, B + BATCH_ * SET * ROW, {}, OK, None, True),
    # two faults: the order (plan, kernels, comps, terms, flags, base_log, shift, rows, batch 0, buffers, sets, overlap)
    ("null-plan-comps-0", NULL, A, E, B, C, dict(comps=0), EINVAL, FN + ": plan is NULL", False),
    ("general-plan-comps-0", GENERAL, A, E, B, C, dict(comps=0), EUNSUPPORTED, T_FUSED, False),
    ("general-plan-null-a", GENERAL, None, E, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("comps-0-terms-0", FUSED, A, E, B, C, dict(comps=0, terms=0), EINVAL, T_COMPS0, False),
    ("comps-3-terms-0", FUSED, A, E, B, C, dict(comps=3, terms=0), EUNSUPPORTED, T_COMPS, False),
    ("comps-3-batch-0", FUSED, None, None, None, None, dict(comps=3, batch=0, sets=1), EUNSUPPORTED, T_COMPS, False),
    ("terms-0-flag-2", FUSED, A, E, B, C, dict(terms=0, flags=2), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2-base-log-0", FUSED, A, E, B, C, dict(flags=2, base_log=0), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0-null-a", FUSED, None, E, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("shift-64-rows", FUSED, 4096, 4096, 4096, 4096, dict(sets=1, batch=2 ** 31, terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-null-a", FUSED, None, 4096, 4096, 4096, dict(sets=1, batch=2 ** 30), EINVAL, T_ROWS, False),
    ("batch0-sets-2", FUSED, A, E, B, C, dict(batch=0, sets=2), OK, None, False),
    ("null-exps-sets-2", FUSED, A, None, B, C, dict(sets=2), EINVAL, FN + ": NULL buffer", False),
    ("sets-2-c-is-a", FUSED, A, E, B, A, dict(sets=2), EINVAL, T_SETS, False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list_of_the_fused_call(cmux, row):
    _, view, a, e, b, c, kw, status, text, launches = row
    full = dict(sets=BATCH_, batch=BATCH_, comps=COMPS, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    st, got, goes_on = cmux.check(view, a, e, b, c, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got


GROUP = 2
M_ROWS = FNM + ": batch * group too large for one call (max 2^31 - 1 rows)"
M_OVERLAP = FNM + ": output must not alias or overlap the input"
# (id, view, a, exps, out, keywords, status, text or None, goes on to a launch)
MONOMIAL_TABLE = [
    ("ok", FUSED, A, E, C, {}, OK, None, True),
    ("general-plan-ok", GENERAL, A, E, C, {}, OK, None, True),
    ("omega-only-plan-ok", OMEGA, A, E, C, {}, OK, None, True),
    ("minus-one-ok", FUSED, A, E, C, dict(flags=1), OK, None, True),
    ("group-1-ok", FUSED, A, E, C, dict(group=1), OK, None, True),
    ("null-plan", NULL, A, E, C, {}, EINVAL, FNM + ": plan is NULL", False),
    ("group-0", FUSED, A, E, C, dict(group=0), EINVAL, FNM + ": group must be at least 1", False),
    ("flag-2", FUSED, A, E, C, dict(flags=2), EINVAL, FNM + ": unknown flag bit", False),
    ("flag-3", FUSED, A, E, C, dict(flags=3), EINVAL, FNM + ": unknown flag bit", False),
    ("rows-2^31", FUSED, 4096, 4096, 4096, dict(batch=2 ** 30), EINVAL, M_ROWS, False),
    ("rows-2^31-minus-2", FUSED, A, E, 1 << 50, dict(batch=2 ** 30 - 1), OK, None, True),
    ("rows-batch-2^63", FUSED, 4096, 4096, 4096, dict(batch=2 ** 63), EINVAL, M_ROWS, False),
    ("rows-group-2^63", FUSED, 4096, 4096, 4096, dict(group=2 ** 63), EINVAL, M_ROWS, False),
    ("batch0-null", FUSED, None, None, None, dict(batch=0), OK, None, False),
    ("null-a", FUSED, None, E, C, {}, EINVAL, FNM + ": NULL buffer", False),
    ("null-exps", FUSED, A, None, C, {}, EINVAL, FNM + ": NULL buffer", False),
    ("null-out", FUSED, A, E, None, {}, EINVAL, FNM + ": NULL buffer", False),
    ("in-place", FUSED, A, E, A, {}, EINVAL, M_OVERLAP, False),
    ("out-over-last-byte-of-a", FUSED, A, E, A + BATCH_ * GROUP * ROW - 1, {}, EINVAL, M_OVERLAP, False),
    ("out-just-past-a", FUSED, A, E, A + BATCH_ * GROUP * ROW, {}, OK, None, True),
    ("out-just-before-a", FUSED, A, E, A - BATCH_ * GROUP * ROW, {}, OK, None, True),
    ("out-past-batch-rows-of-a", FUSED, A, E, A + BATCH_ * ROW, {}, EINVAL, M_OVERLAP, False),
    # two faults: the order (plan, group, flags, rows, batch 0, buffers, overlap)
    ("null-plan-group-0", NULL, A, E, C, dict(group=0), EINVAL, FNM + ": plan is NULL", False),
    ("group-0-flag-2", FUSED, A, E, C, dict(group=0, flags=2), EINVAL, FNM + ": group must be at least 1", False),
    ("flag-2-rows", FUSED, 4096, 4096, 4096, dict(flags=2, batch=2 ** 30), EINVAL, FNM + ": unknown flag bit", False),
    ("flag-2-batch-0", FUSED, None, None, None, dict(flags=2, batch=0), EINVAL, FNM + ": unknown flag bit", False),
    ("rows-null-a", FUSED, None, 4096, 4096, dict(batch=2 ** 30), EINVAL, M_ROWS, False),
    ("null-a-in-place", FUSED, None, E, None, {}, EINVAL, FNM + ": NULL buffer", False),
]


@pytest.mark.parametrize("row", MONOMIAL_TABLE, ids=[r[0] for r in MONOMIAL_TABLE])
def test_argument_list_of_the_monomial_call(cmux, row):
    _, view, a, e, out, kw, status, text, launches = row
    full = dict(batch=BATCH_, group=GROUP, flags=0)
    full.update(kw)
    st, got, goes_on = cmux.check_monomial(view, a, e, out, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got
