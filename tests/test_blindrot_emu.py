"""CPU stepping of the blind-rotation kernel (tests/emu/emu_blindrot.cpp: polydot_blindrot_kernel stepped thread by
thread with the kernel's own headers, the accumulator in an LDS image across steps and rows, every access to it checked against
the step it belongs to) against the loop it replaces (one stepped CMux rotation per step, tests/emu/emu_cmux.cpp, on a shared key),
against an algebraic identity that does not pass through the project's decomposition, and the entry point's argument list
(csrc/api_checks.h: check_blind_rotate) with the LDS rule (csrc/launch_plan.h), without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import p64
from test_cmux_emu import EmuCmux, TRIVIAL, exponents, monomial_np, trivial_key
from test_dot_emu import sum_mod
from test_extprod_emu import digit_rows, input_rows
from test_gadget_emu import MODES, POLICIES, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data, shape_params

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FN, LOOP = "tn_poly_blind_rotate_prepared_dev", "tn_poly_cmux_rotate_prepared_dev"
BATCH, STEPS = 7, 3
P32 = ctypes.POINTER(ctypes.c_uint32)
WG_LDS = 160 * 1024


def step_exponents(n, steps, batch=BATCH, seed=0):
    """(steps, batch): step 0 has the exponents of tests/test_cmux_emu.py (batch 7), later steps seeded random 32-bit words."""
    rng = np.random.default_rng(1000 + n + seed)
    e = rng.integers(0, 2 ** 32, (steps, batch), dtype=np.uint64).astype(np.uint32)
    if batch == BATCH:
        e[0] = exponents(n)
    return e


def step_key_rows(steps, terms):
    """Rows of a case's b for the keys, one shared key per step: b[(k + o + 2 * i + 3 * j) % 5] is term j of input i of component o
    of step k -> (steps, 2, 2, terms)."""
    return np.array([[[[(k + o + 2 * i + 3 * j) % 5 for j in range(terms)] for i in range(2)] for o in range(2)] for k in range(steps)])


class EmuBlindrot:
    """The entry points of tests/emu/emu_blindrot.cpp in tests/emu/_build/libemu.so."""

    def __init__(self):
        L = self.lib = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        P64 = ctypes.POINTER(ctypes.c_uint64)
        L.emu_poly_blind_rotate_prepared.argtypes = [u32, u64, u64, ci, P64, P32, P64, P64, sz, sz, sz, u32, u32]
        L.emu_blindrot_lds_fits.argtypes = [u32, ci, ci, ctypes.POINTER(sz), ctypes.POINTER(ci)]
        L.emu_blindrot_api_check.argtypes = [u32, ci, ci, ci, u64, ci, vp, vp, vp, vp, sz, sz, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]

    def rotate_code(self, n, q, psi, a, exps, bhat, terms, w, balanced=False, canonical=False):
        """a: (batch, 2, n); exps: (steps, batch); bhat: (steps * 4 * terms, n) -> (return code, (batch, 2, n))."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.shape[0]
        assert a.shape[1:] == (2, n)
        e = np.ascontiguousarray(exps, dtype=np.uint32)
        steps = e.shape[0]
        assert e.shape == (steps, batch)
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] == steps * 4 * terms
        c = np.empty((batch, 2, n), dtype=np.uint64)
        rc = self.lib.emu_poly_blind_rotate_prepared(n, q, psi, int(canonical), p64(a), e.ctypes.data_as(P32), p64(bhat), p64(c), batch, steps, terms, w,
                                                     int(balanced))
        return rc, c

    def rotate(self, *args, **kw):
        rc, c = self.rotate_code(*args, **kw)
        assert rc == 0, rc
        return c

    def lds(self, n, elem_bytes, lazy):
        """-> (supported, the workgroup's LDS request in bytes, input words per thread put away)."""
        b, w = ctypes.c_size_t(0), ctypes.c_int(0)
        fits = self.lib.emu_blindrot_lds_fits(n, elem_bytes, int(lazy), ctypes.byref(b), ctypes.byref(w))
        return bool(fits), b.value, w.value

    def check(self, view, a, e, b, c, batch=1, comps=2, steps=1, terms=1, base_log=1, flags=0):
        """check_blind_rotate on the plan view (n, elem_bytes, has_fused, omega_only, q, lazy) -> (status, text, goes on to a launch)."""
        return emu_library.api_check(self.lib.emu_blindrot_api_check, *view, a, e, b, c, batch, comps, steps, terms, base_log, flags)


@pytest.fixture(scope="module")
def blindrot():
    return EmuBlindrot()


@pytest.fixture(scope="module")
def cmux():
    return EmuCmux()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def loop_of_steps(cmux, n, q, psi, a, exps, bh, terms, w, balanced, canonical):
    """The loop the call replaces: one stepped CMux rotation per step on the step's shared key -> the accumulator after every step."""
    out, acc = [], a
    for k in range(exps.shape[0]):
        acc = cmux.rotate(n, q, psi, acc, exps[k], bh[k * 4 * terms:(k + 1) * 4 * terms], terms, w, balanced, canonical)
        out.append(acc)
    return out


def supported(blindrot, case, canonical):
    n, q, _ = shape_params(case)
    return blindrot.lds(n, 4 if q < 2 ** 31 else 8, not canonical)[0]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepped_blind_rotation_is_the_loop_of_stepped_rotations(blindrot, cmux, prep, case, canonical):
    """Batch 7 (one emulated workgroup reloads the LDS accumulator six times), three steps, every (terms, w) of gadget_pairs, both
    digit modes: the one call equals three stepped CMux rotations on the steps' keys, and with one step it equals one.  A shape
    the LDS rule refuses is refused by the stepping (code 8) and by the argument list, which names the loop."""
    n, q, psi, a, b = _case_data(case)
    word = 4 if q < 2 ** 31 else 8
    if not supported(blindrot, case, canonical):
        rc, _ = blindrot.rotate_code(n, q, psi, np.zeros((1, 2, n), dtype=np.uint64), np.zeros((1, 1), dtype=np.uint32), np.zeros((4, n), dtype=np.uint64), 1, 1,
                                     False, canonical)
        assert rc == 8
        st, text, goes_on = blindrot.check((n, word, 1, 0, q, int(not canonical)), 1 << 20, 1 << 44, 1 << 30, 1 << 40)
        assert (st, goes_on) == (EUNSUPPORTED, False) and text.startswith(FN + ": ") and LOOP in text, text
        return
    st, text, goes_on = blindrot.check((n, word, 1, 0, q, int(not canonical)), 1 << 20, 1 << 44, 1 << 30, 1 << 40)
    assert (st, text, goes_on) == (OK, "", True)
    bhat = prep.prepare(n, q, psi, b, canonical)
    exps = step_exponents(n, STEPS)
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        a7 = np.ascontiguousarray(a[input_rows(BATCH, 2, first)])        # (7, 2, n)
        bh = bhat[step_key_rows(STEPS, terms).ravel()]
        for balanced in MODES:
            where = (case, canonical, terms, w, balanced)
            ref = loop_of_steps(cmux, n, q, psi, a7, exps, bh, terms, w, balanced, canonical)
            assert np.array_equal(blindrot.rotate(n, q, psi, a7, exps, bh, terms, w, balanced, canonical), ref[-1]), where
            assert np.array_equal(blindrot.rotate(n, q, psi, a7, exps[:1], bh[:4 * terms], terms, w, balanced, canonical), ref[0]), where


@POLICIES
def test_trivial_rgsw_keys_of_bits_rotate_by_the_selected_sum(blindrot, prep, canonical):
    """Uses none of the project's decomposition: with noise-free trivial RGSW keys of bits m_k (unsigned digits that cover q
    recompose exactly) step k multiplies the accumulator by X^(m_k e_k), so nine steps return rot_E(a mod q) with
    E = sum m_k e_k mod 2n, word for word."""
    n, q, psi, a, _ = _case_data("P256")
    steps = 9
    terms, w = TRIVIAL[q.bit_length()]
    assert terms * w >= q.bit_length() and (1 << w) < q and (terms - 1) * w < 64
    bits = np.random.default_rng(256).integers(0, 2, steps)
    bits[0], bits[1] = 1, 0                                                # both values whatever the seed gives
    assert set(int(m) for m in bits) == {0, 1}
    keys = {m: prep.prepare(n, q, psi, trivial_key(n, q, m, terms, w), canonical) for m in (0, 1)}
    bh = np.concatenate([keys[int(m)] for m in bits])
    exps = step_exponents(n, steps)
    a7 = np.ascontiguousarray(a[input_rows(BATCH, 2)])
    total = [sum(int(bits[k]) * int(exps[k, r]) for k in range(steps)) % (2 * n) for r in range(BATCH)]
    assert len(set(total)) > 1
    c = blindrot.rotate(n, q, psi, a7, exps, bh, terms, w, False, canonical)
    assert np.array_equal(c, monomial_np(a7, total, q)), canonical


@pytest.mark.parametrize("case", ["P256", "P4096_60"])
@POLICIES
def test_two_steps_match_the_oracle_products_of_the_python_digits(blindrot, prep, oracle, case, canonical):
    """Uses none of the stepping's own digit cut or term step: per step and component, the accumulator mod q plus the sum mod q
    of the oracle's products of the Python-decomposed digits of the numpy monomial product, both digit modes.  The comparison
    with the loop of stepped CMux rotations above runs the same term step on both sides (gadget_term_step, tests/emu/emu_stepper.h),
    so a slip in the step's carries shows here."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    steps = 2
    exps = step_exponents(n, steps)
    a7 = np.ascontiguousarray(a[input_rows(BATCH, 2)])
    terms, w = gadget_pairs(q)[0]
    idx = step_key_rows(steps, terms)                                       # (steps, 2, 2, terms) rows of b
    for balanced in MODES:
        acc = a7 % np.uint64(q)
        for k in range(steps):
            digits = digit_rows(monomial_np(acc, exps[k], q, True), q, w, terms, balanced).reshape(-1, n)
            step = np.empty_like(acc)
            for o in range(2):
                prods = oracle.poly_mult(digits, b[np.tile(idx[k, o].ravel(), BATCH)], q, psi).reshape(BATCH, 2 * terms, n)
                step[:, o] = (acc[:, o] + sum_mod(prods, q)) % np.uint64(q)
            acc = step
        c = blindrot.rotate(n, q, psi, a7, exps, bhat[idx.ravel()], terms, w, balanced, canonical)
        assert np.array_equal(c, acc), (case, canonical, balanced)


def test_lds_rule_over_every_shape(blindrot):
    """The request is the transpose image, the words put away, two rows of n words, two staged tables and the slot; a shape is
    supported when it is at most 160 KiB.  Over the limit: n = 8192 with 64-bit words, alone."""
    refused = []
    for word in (4, 8):
        for lazy in (False, True):
            for logn in range(6, 16):
                n = 1 << logn
                fits, req, words = blindrot.lds(n, word, lazy)
                if 8 <= logn <= 13:
                    assert req > 3 * n * word and 0 <= words <= 8, (n, word, lazy, req, words)
                    assert fits == (req <= WG_LDS), (n, word, lazy, req)
                    if not fits:
                        refused.append((n, word))
                else:
                    assert (fits, req, words) == (False, 0, 0), (n, word, lazy)
    assert sorted(set(refused)) == [(8192, 8)]


# ---- the argument list -------------------------------------------------------------------------
N, WORD, Q, W = 256, 4, 8380417, 4                          # the smallest fused plan: rows of 1 KiB; 2^W < Q
ROW = N * WORD
FUSED, GENERAL, NULL = (N, WORD, 1, 0, Q, 1), (N, WORD, 0, 0, Q, 0), (0, 0, 0, 0, 0, 0)
OVER = (8192, 8, 1, 0, 1152921504606830593, 1)              # fused kernels, but the accumulator does not fit
A, B, C, E = 1 << 24, 1 << 30, 1 << 40, 1 << 44
BATCH_, COMPS, STEPS_, TERMS = 5, 2, 3, 2
ACC = BATCH_ * COMPS                                        # rows of a and of c
KEYS = STEPS_ * COMPS * COMPS * TERMS                       # rows of bhat
T_FUSED = FN + ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_SHAPE = FN + ": the accumulator of this shape does not fit a workgroup's LDS (loop over tn_poly_cmux_rotate_prepared_dev)"
T_COMPS0 = FN + ": comps must be 2"
T_COMPS = FN + ": comps other than 2 is not supported (tn_monomial_mul_dev, tn_poly_external_product_prepared_dev, then an addition)"
T_STEPS = FN + ": steps must be at least 1"
T_BASE = FN + ": need 1 <= base_log and 2^base_log < q"
T_KEY_ROWS = FN + ": steps * 4 * terms too large for one call (max 2^31 - 1 key rows)"
T_ACC_ROWS = FN + ": batch * 2 too large for one call (max 2^31 - 1 accumulator rows)"
T_EXPS = FN + ": steps * batch too large for one call (max 2^31 - 1 exponents)"
T_SAME = FN + ": c may be a itself (in place) but must not overlap it otherwise"
T_KEY = FN + ": output must not alias or overlap the key"

# (id, view, a, exps, bhat, c, keywords, status, text or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, E, B, C, {}, OK, None, True),
    ("balanced-ok", FUSED, A, E, B, C, dict(flags=1), OK, None, True),
    ("in-place-ok", FUSED, A, E, B, A, {}, OK, None, True),
    ("one-step-ok", FUSED, A, E, B, C, dict(steps=1), OK, None, True),
    # one row per fault, in the order of the list
    ("null-plan", NULL, A, E, B, C, {}, EINVAL, FN + ": plan is NULL", False),
    ("general-plan", GENERAL, A, E, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("shape-over-lds", OVER, A, E, B, C, dict(base_log=30), EUNSUPPORTED, T_SHAPE, False),
    ("comps-0", FUSED, A, E, B, C, dict(comps=0), EINVAL, T_COMPS0, False),
    ("comps-1", FUSED, A, E, B, C, dict(comps=1), EUNSUPPORTED, T_COMPS, False),
    ("comps-3", FUSED, A, E, B, C, dict(comps=3), EUNSUPPORTED, T_COMPS, False),
    ("steps-0", FUSED, A, E, B, C, dict(steps=0), EINVAL, T_STEPS, False),
    ("terms-0", FUSED, A, E, B, C, dict(terms=0), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2", FUSED, A, E, B, C, dict(flags=2), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0", FUSED, A, E, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("base-log-k", FUSED, A, E, B, C, dict(base_log=23), EINVAL, T_BASE, False),
    ("shift-64", FUSED, A, E, B, C, dict(terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("key-rows-2^31", FUSED, 4096, 4096, 4096, 4096, dict(steps=2 ** 28, terms=2, base_log=1), EINVAL, T_KEY_ROWS, False),
    ("key-rows-steps-2^63", FUSED, 4096, 4096, 4096, 4096, dict(steps=2 ** 63, terms=1), EINVAL, T_KEY_ROWS, False),
    ("key-rows-2^31-minus-4", FUSED, A, E, 1 << 50, 1 << 62, dict(steps=2 ** 29 - 1, terms=1, batch=1), OK, None, True),
    ("acc-rows-2^31", FUSED, 4096, 4096, 4096, 4096, dict(batch=2 ** 30, steps=1), EINVAL, T_ACC_ROWS, False),
    ("acc-rows-batch-2^63", FUSED, 4096, 4096, 4096, 4096, dict(batch=2 ** 63, steps=1), EINVAL, T_ACC_ROWS, False),
    ("exponents-2^31", FUSED, 4096, 4096, 4096, 4096, dict(batch=2 ** 16, steps=2 ** 15), EINVAL, T_EXPS, False),
    ("exponents-2^31-minus", FUSED, A, E, 1 << 50, 1 << 62, dict(batch=2 ** 16 - 1, steps=2 ** 15), OK, None, True),
    ("batch0-null", FUSED, None, None, None, None, dict(batch=0), OK, None, False),
    ("null-a", FUSED, None, E, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-exps", FUSED, A, None, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-bhat", FUSED, A, E, None, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-c", FUSED, A, E, B, None, {}, EINVAL, FN + ": NULL buffer", False),
    # overlap by byte range: c's batch * 2 rows against a's batch * 2 rows, the same pointer excepted ...
    ("c-one-byte-past-a", FUSED, A, E, B, A + 1, {}, EINVAL, T_SAME, False),
    ("c-one-row-past-a", FUSED, A, E, B, A + ROW, {}, EINVAL, T_SAME, False),
    ("c-over-last-row-of-a", FUSED, A, E, B, A + (ACC - 1) * ROW, {}, EINVAL, T_SAME, False),
    ("c-last-byte-is-first-of-a", FUSED, A, E, B, A - ACC * ROW + 1, {}, EINVAL, T_SAME, False),
    ("c-just-before-a", FUSED, A, E, B, A - ACC * ROW, {}, OK, None, True),
    ("c-over-last-byte-of-a", FUSED, A, E, B, A + ACC * ROW - 1, {}, EINVAL, T_SAME, False),
    ("c-just-past-a", FUSED, A, E, B, A + ACC * ROW, {}, OK, None, True),
    # ... and against the steps * 4 * terms rows of the keys
    ("c-is-the-key", FUSED, A, E, B, B, {}, EINVAL, T_KEY, False),
    ("c-over-first-row-of-the-keys", FUSED, A, E, B, B - (ACC - 1) * ROW, {}, EINVAL, T_KEY, False),
    ("c-just-before-the-keys", FUSED, A, E, B, B - ACC * ROW, {}, OK, None, True),
    ("c-past-the-first-key", FUSED, A, E, B, B + COMPS * COMPS * TERMS * ROW, {}, EINVAL, T_KEY, False),
    ("c-over-last-row-of-the-keys", FUSED, A, E, B, B + (KEYS - 1) * ROW, {}, EINVAL, T_KEY, False),
    ("c-just-past-the-keys", FUSED, A, E, B, B + KEYS * ROW, {}, OK, None, True),
    ("in-place-over-the-keys", FUSED, B, E, B, B, {}, EINVAL, T_KEY, False),
    # two faults: the order (plan, kernels, shape, comps, steps, terms, flags, base_log, shift, key rows, accumulator rows,
    # exponents, batch 0, buffers, c against a, c against the keys)
    ("null-plan-comps-0", NULL, A, E, B, C, dict(comps=0), EINVAL, FN + ": plan is NULL", False),
    ("general-plan-comps-0", GENERAL, A, E, B, C, dict(comps=0), EUNSUPPORTED, T_FUSED, False),
    ("shape-comps-0", OVER, A, E, B, C, dict(comps=0), EUNSUPPORTED, T_SHAPE, False),
    ("shape-batch-0", OVER, None, None, None, None, dict(batch=0), EUNSUPPORTED, T_SHAPE, False),
    ("comps-0-steps-0", FUSED, A, E, B, C, dict(comps=0, steps=0), EINVAL, T_COMPS0, False),
    ("comps-3-steps-0", FUSED, A, E, B, C, dict(comps=3, steps=0), EUNSUPPORTED, T_COMPS, False),
    ("steps-0-terms-0", FUSED, A, E, B, C, dict(steps=0, terms=0), EINVAL, T_STEPS, False),
    ("steps-0-batch-0", FUSED, None, None, None, None, dict(steps=0, batch=0), EINVAL, T_STEPS, False),
    ("terms-0-flag-2", FUSED, A, E, B, C, dict(terms=0, flags=2), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2-base-log-0", FUSED, A, E, B, C, dict(flags=2, base_log=0), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0-null-a", FUSED, None, E, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("key-rows-acc-rows", FUSED, 4096, 4096, 4096, 4096, dict(steps=2 ** 29, terms=1, batch=2 ** 30), EINVAL, T_KEY_ROWS, False),
    ("acc-rows-exponents", FUSED, 4096, 4096, 4096, 4096, dict(batch=2 ** 30, steps=2), EINVAL, T_ACC_ROWS, False),
    ("exponents-null-a", FUSED, None, 4096, 4096, 4096, dict(batch=2 ** 16, steps=2 ** 15), EINVAL, T_EXPS, False),
    ("batch0-c-over-a", FUSED, A, E, B, A + 1, dict(batch=0), OK, None, False),
    ("null-exps-c-over-a", FUSED, A, None, B, A + 1, {}, EINVAL, FN + ": NULL buffer", False),
    ("c-over-a-and-the-keys", FUSED, A, E, A + ROW, A + ROW, {}, EINVAL, T_SAME, False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(blindrot, row):
    _, view, a, e, b, c, kw, status, text, launches = row
    full = dict(batch=BATCH_, comps=COMPS, steps=STEPS_, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    st, got, goes_on = blindrot.check(view, a, e, b, c, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got
