"""The argument lists of tn_lwe_modswitch_dev, tn_sample_extract_dev and tn_lwe_keyswitch_dev (tiny_ntt_amd/csrc/api_checks.h:
check_lwe_modswitch, check_sample_extract, check_lwe_keyswitch, the lists capi.cpp runs) on the CPU: one row per branch, in the
order of the list, then rows with two faults that pin the order, then the overlap rule byte by byte.  No pointer is read."""
import pytest

import lwe_cases as L

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
N, WORD, Q = 4, 4, 7681                                     # the smallest plan; 2^W < Q
PLAN, GENERAL, OMEGA, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (N, WORD, 0, 1, Q), (0, 0, 0, 0, 0)
WIDE = (N, 8, 1, 0, (1 << 60) - (1 << 14) + 1)              # 64-bit words: base_log up to 59 passes the gadget rule
A, B, C = 1 << 20, 1 << 30, 1 << 40
MS, SE, KS = "tn_lwe_modswitch_dev: ", "tn_sample_extract_dev: ", "tn_lwe_keyswitch_dev: "
T_DIM = "dim must be between 1 and TN_LWE_MAX_DIM (65536)"
T_NIN = "n_in must be between 1 and TN_LWE_MAX_DIM (65536)"
T_NOUT = "n_out must be between 1 and TN_LWE_MAX_DIM (65536)"
T_BASE = "need 1 <= base_log and 2^base_log < q"
T_W32 = "base_log above 32 is not supported: the kernel keeps digits as 32-bit words (LWE key switches use bases of 2^2 to 2^8)"
T_IN = "output must not alias or overlap the input"
T_ANY = "output must not alias or overlap an input"


@pytest.fixture(scope="module")
def emu():
    return L.emu_lwe()


def words(name):
    return f"batch * ({name} + 1) too large for one call (max 2^31 - 1 words)"


BATCH, DIM = 3, 5
# (id, view, lwe, exps, batch, dim, status, text, goes on to a launch)
MODSWITCH = [
    ("ok", PLAN, A, B, BATCH, DIM, OK, "", True),
    ("general-plan-ok", GENERAL, A, B, BATCH, DIM, OK, "", True),
    ("omega-plan-ok", OMEGA, A, B, BATCH, DIM, OK, "", True),
    ("dim-max-ok", PLAN, A, B, BATCH, 65536, OK, "", True),
    ("null-plan", NULL, A, B, BATCH, DIM, EINVAL, MS + "plan is NULL", False),
    ("dim-0", PLAN, A, B, BATCH, 0, EINVAL, MS + T_DIM, False),
    ("dim-above", PLAN, A, B, BATCH, 65537, EINVAL, MS + T_DIM, False),
    ("words-2^31", PLAN, A, B, 2 ** 30, 1, EINVAL, MS + words("dim"), False),
    ("words-2^31-minus-1", PLAN, 4096, 1 << 50, (2 ** 31 - 1) // 3, 2, OK, "", True),
    ("batch-2^63", PLAN, A, B, 2 ** 63, 1, EINVAL, MS + words("dim"), False),
    ("batch0-null", PLAN, None, None, 0, DIM, OK, "", False),
    ("null-lwe", PLAN, None, B, BATCH, DIM, EINVAL, MS + "NULL buffer", False),
    ("null-exps", PLAN, A, None, BATCH, DIM, EINVAL, MS + "NULL buffer", False),
    ("exps-is-lwe", PLAN, A, A, BATCH, DIM, EINVAL, MS + T_IN, False),
    ("exps-over-last-byte", PLAN, A, A + BATCH * (DIM + 1) * WORD - 1, BATCH, DIM, EINVAL, MS + T_IN, False),
    ("exps-just-past", PLAN, A, A + BATCH * (DIM + 1) * WORD, BATCH, DIM, OK, "", True),
    ("exps-just-before", PLAN, A, A - BATCH * (DIM + 1) * 4, BATCH, DIM, OK, "", True),
    ("exps-last-byte-is-first", PLAN, A, A - BATCH * (DIM + 1) * 4 + 1, BATCH, DIM, EINVAL, MS + T_IN, False),
    ("wide-exps-inside-lwe", WIDE, A, A + BATCH * (DIM + 1) * 8 - 1, BATCH, DIM, EINVAL, MS + T_IN, False),
    ("wide-exps-just-past", WIDE, A, A + BATCH * (DIM + 1) * 8, BATCH, DIM, OK, "", True),
    # two faults: the order (plan, dim, words, batch 0, buffers, overlap)
    ("null-plan-dim-0", NULL, A, B, BATCH, 0, EINVAL, MS + "plan is NULL", False),
    ("dim-0-words", PLAN, A, B, 2 ** 31, 0, EINVAL, MS + T_DIM, False),
    ("dim-0-batch-0", PLAN, None, None, 0, 0, EINVAL, MS + T_DIM, False),
    ("words-null", PLAN, None, None, 2 ** 31, 1, EINVAL, MS + words("dim"), False),
    ("batch0-overlap", PLAN, A, A, 0, DIM, OK, "", False),
    ("null-overlap", PLAN, None, None, BATCH, DIM, EINVAL, MS + "NULL buffer", False),
]


@pytest.mark.parametrize("row", MODSWITCH, ids=[r[0] for r in MODSWITCH])
def test_modswitch_argument_list(emu, row):
    _, view, lwe, exps, batch, dim, status, text, launches = row
    st, got, goes_on = emu.check("modswitch", view, lwe, exps, batch, dim)
    assert (st, goes_on, got) == (status, launches, text)


A_BYTES = BATCH * 2 * N * WORD
# (id, view, a, lwe, batch, index, status, text, launches)
EXTRACT = [
    ("ok", PLAN, A, B, BATCH, 0, OK, "", True),
    ("general-plan-ok", GENERAL, A, B, BATCH, 1, OK, "", True),
    ("omega-plan-ok", OMEGA, A, B, BATCH, 1, OK, "", True),
    ("last-index-ok", PLAN, A, B, BATCH, N - 1, OK, "", True),
    ("null-plan", NULL, A, B, BATCH, 0, EINVAL, SE + "plan is NULL", False),
    ("index-n", PLAN, A, B, BATCH, N, EINVAL, SE + "index must be below n", False),
    ("index-all-ones", PLAN, A, B, BATCH, 2 ** 32 - 1, EINVAL, SE + "index must be below n", False),
    ("words-2^31", PLAN, A, B, 2 ** 29, 0, EINVAL, SE + words("n"), False),
    ("batch-2^63", PLAN, A, B, 2 ** 63, 0, EINVAL, SE + words("n"), False),
    ("batch0-null", PLAN, None, None, 0, 0, OK, "", False),
    ("null-a", PLAN, None, B, BATCH, 0, EINVAL, SE + "NULL buffer", False),
    ("null-lwe", PLAN, A, None, BATCH, 0, EINVAL, SE + "NULL buffer", False),
    ("lwe-is-a", PLAN, A, A, BATCH, 0, EINVAL, SE + T_IN, False),
    ("lwe-over-last-byte-of-a", PLAN, A, A + A_BYTES - 1, BATCH, 0, EINVAL, SE + T_IN, False),
    ("lwe-just-past-a", PLAN, A, A + A_BYTES, BATCH, 0, OK, "", True),
    ("lwe-just-before-a", PLAN, A, A - BATCH * (N + 1) * WORD, BATCH, 0, OK, "", True),
    ("lwe-last-byte-is-first-of-a", PLAN, A, A - BATCH * (N + 1) * WORD + 1, BATCH, 0, EINVAL, SE + T_IN, False),
    # two faults: the order (plan, index, words, batch 0, buffers, overlap)
    ("null-plan-index-n", NULL, A, B, BATCH, N, EINVAL, SE + "plan is NULL", False),
    ("index-n-words", PLAN, A, B, 2 ** 31, N, EINVAL, SE + "index must be below n", False),
    ("index-n-batch-0", PLAN, None, None, 0, N, EINVAL, SE + "index must be below n", False),
    ("words-null", PLAN, None, None, 2 ** 31, 0, EINVAL, SE + words("n"), False),
    ("batch0-overlap", PLAN, A, A, 0, 0, OK, "", False),
    ("null-overlap", PLAN, None, None, BATCH, 0, EINVAL, SE + "NULL buffer", False),
]


@pytest.mark.parametrize("row", EXTRACT, ids=[r[0] for r in EXTRACT])
def test_sample_extract_argument_list(emu, row):
    _, view, a, lwe, batch, index, status, text, launches = row
    st, got, goes_on = emu.check("extract", view, a, lwe, batch, index)
    assert (st, goes_on, got) == (status, launches, text)


NIN, NOUT, TERMS, W = 8, 5, 2, 4
LWE_BYTES, OUT_BYTES, KSK_BYTES = BATCH * (NIN + 1) * WORD, BATCH * (NOUT + 1) * WORD, NIN * TERMS * (NOUT + 1) * WORD
# (id, view, lwe, ksk, out, keywords, status, text, launches)
KEYSWITCH = [
    ("ok", PLAN, A, B, C, {}, OK, "", True),
    ("balanced-ok", PLAN, A, B, C, dict(flags=1), OK, "", True),
    ("general-plan-ok", GENERAL, A, B, C, {}, OK, "", True),
    ("omega-plan-ok", OMEGA, A, B, C, {}, OK, "", True),
    ("dims-1-ok", PLAN, A, B, C, dict(n_in=1, n_out=1), OK, "", True),
    ("dims-max-ok", PLAN, A, B, 1 << 50, dict(n_in=65536, n_out=65536, terms=3), OK, "", True),
    ("base-log-32-ok", WIDE, A, B, C, dict(base_log=32), OK, "", True),
    ("2^22-terms-ok", PLAN, A, B, 1 << 50, dict(n_in=65536, terms=64, base_log=1), OK, "", True),
    # one row per fault, in the order of the list
    ("null-plan", NULL, A, B, C, {}, EINVAL, KS + "plan is NULL", False),
    ("n-in-0", PLAN, A, B, C, dict(n_in=0), EINVAL, KS + T_NIN, False),
    ("n-in-above", PLAN, A, B, C, dict(n_in=65537), EINVAL, KS + T_NIN, False),
    ("n-out-0", PLAN, A, B, C, dict(n_out=0), EINVAL, KS + T_NOUT, False),
    ("n-out-above", PLAN, A, B, C, dict(n_out=65537), EINVAL, KS + T_NOUT, False),
    ("terms-0", PLAN, A, B, C, dict(terms=0), EINVAL, KS + "terms must be at least 1", False),
    ("flag-2", PLAN, A, B, C, dict(flags=2), EINVAL, KS + "unknown flag bit", False),
    ("base-log-0", PLAN, A, B, C, dict(base_log=0), EINVAL, KS + T_BASE, False),
    ("base-log-k", PLAN, A, B, C, dict(base_log=13), EINVAL, KS + T_BASE, False),
    ("base-log-64", WIDE, A, B, C, dict(base_log=64), EINVAL, KS + T_BASE, False),
    ("shift-64", PLAN, A, B, C, dict(terms=65, base_log=1), EINVAL, KS + "(terms - 1) * base_log must be below 64", False),
    ("base-log-33", WIDE, A, B, C, dict(base_log=33, terms=1), EUNSUPPORTED, KS + T_W32, False),
    ("base-log-59", WIDE, A, B, C, dict(base_log=59, terms=2), EUNSUPPORTED, KS + T_W32, False),
    ("lwe-words-2^31", PLAN, A, B, C, dict(batch=2 ** 28), EINVAL, KS + words("n_in"), False),
    ("out-words-2^31", PLAN, A, B, C, dict(batch=2 ** 28, n_in=1, n_out=7), EINVAL, KS + words("n_out"), False),
    ("batch-2^63", PLAN, A, B, C, dict(batch=2 ** 63), EINVAL, KS + words("n_in"), False),
    ("batch0-null", PLAN, None, None, None, dict(batch=0), OK, "", False),
    ("null-lwe", PLAN, None, B, C, {}, EINVAL, KS + "NULL buffer", False),
    ("null-ksk", PLAN, A, None, C, {}, EINVAL, KS + "NULL buffer", False),
    ("null-out", PLAN, A, B, None, {}, EINVAL, KS + "NULL buffer", False),
    ("out-is-lwe", PLAN, A, B, A, {}, EINVAL, KS + T_ANY, False),
    ("out-over-last-byte-of-lwe", PLAN, A, B, A + LWE_BYTES - 1, {}, EINVAL, KS + T_ANY, False),
    ("out-just-past-lwe", PLAN, A, B, A + LWE_BYTES, {}, OK, "", True),
    ("out-just-before-lwe", PLAN, A, B, A - OUT_BYTES, {}, OK, "", True),
    ("out-last-byte-is-first-of-lwe", PLAN, A, B, A - OUT_BYTES + 1, {}, EINVAL, KS + T_ANY, False),
    ("out-is-ksk", PLAN, A, B, B, {}, EINVAL, KS + T_ANY, False),
    ("out-over-last-byte-of-ksk", PLAN, A, B, B + KSK_BYTES - 1, {}, EINVAL, KS + T_ANY, False),
    ("out-just-past-ksk", PLAN, A, B, B + KSK_BYTES, {}, OK, "", True),
    ("out-just-before-ksk", PLAN, A, B, B - OUT_BYTES, {}, OK, "", True),
    # two faults: the order (plan, n_in, n_out, terms, flags, base_log, shift, key rows, digits, words of lwe, of out, batch 0,
    # buffers, overlap)
    ("null-plan-n-in-0", NULL, A, B, C, dict(n_in=0), EINVAL, KS + "plan is NULL", False),
    ("n-in-0-n-out-0", PLAN, A, B, C, dict(n_in=0, n_out=0), EINVAL, KS + T_NIN, False),
    ("n-out-0-terms-0", PLAN, A, B, C, dict(n_out=0, terms=0), EINVAL, KS + T_NOUT, False),
    ("terms-0-flag-2", PLAN, A, B, C, dict(terms=0, flags=2), EINVAL, KS + "terms must be at least 1", False),
    ("flag-2-base-log-0", PLAN, A, B, C, dict(flags=2, base_log=0), EINVAL, KS + "unknown flag bit", False),
    ("base-log-64-before-33", WIDE, A, B, C, dict(base_log=64, terms=1), EINVAL, KS + T_BASE, False),
    ("shift-before-digits", WIDE, A, B, C, dict(base_log=33, terms=3), EINVAL, KS + "(terms - 1) * base_log must be below 64", False),
    ("digits-before-words", WIDE, A, B, C, dict(base_log=33, terms=1, batch=2 ** 31), EUNSUPPORTED, KS + T_W32, False),
    ("digits-before-batch-0", WIDE, None, None, None, dict(base_log=33, terms=1, batch=0), EUNSUPPORTED, KS + T_W32, False),
    ("lwe-words-before-out-words", PLAN, A, B, C, dict(batch=2 ** 31), EINVAL, KS + words("n_in"), False),
    ("words-null", PLAN, None, None, None, dict(batch=2 ** 31), EINVAL, KS + words("n_in"), False),
    ("base-log-0-null", PLAN, None, B, C, dict(base_log=0), EINVAL, KS + T_BASE, False),
    ("batch0-overlap", PLAN, A, B, A, dict(batch=0), OK, "", False),
    ("null-overlap", PLAN, None, B, B, {}, EINVAL, KS + "NULL buffer", False),
]


@pytest.mark.parametrize("row", KEYSWITCH, ids=[r[0] for r in KEYSWITCH])
def test_keyswitch_argument_list(emu, row):
    _, view, lwe, ksk, out, kw, status, text, launches = row
    full = dict(batch=BATCH, n_in=NIN, n_out=NOUT, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    st, got, goes_on = emu.check("keyswitch", view, lwe, ksk, out, full["batch"], full["n_in"], full["n_out"], full["terms"], full["base_log"],
                                 full["flags"])
    assert (st, goes_on, got) == (status, launches, text)


def test_overlap_is_the_intersection_of_the_byte_ranges(emu):
    """Every half word around the inputs: exps against lwe, lwe against a, out against lwe and against ksk."""
    for off in range(-2 * LWE_BYTES, 2 * KSK_BYTES, 2):
        out = A + off
        want = out < A + LWE_BYTES and A < out + OUT_BYTES
        st, text, goes_on = emu.check("keyswitch", PLAN, A, B, out, BATCH, NIN, NOUT, TERMS, W, 0)
        assert (st, goes_on, text) == ((EINVAL, False, KS + T_ANY) if want else (OK, True, "")), off
        want = out < A + KSK_BYTES and A < out + OUT_BYTES
        st, text, goes_on = emu.check("keyswitch", PLAN, B, A, out, BATCH, NIN, NOUT, TERMS, W, 0)
        assert (st, goes_on, text) == ((EINVAL, False, KS + T_ANY) if want else (OK, True, "")), off
        want = out < A + BATCH * (DIM + 1) * WORD and A < out + BATCH * (DIM + 1) * 4
        st, text, goes_on = emu.check("modswitch", PLAN, A, out, BATCH, DIM)
        assert (st, goes_on, text) == ((EINVAL, False, MS + T_IN) if want else (OK, True, "")), off
        want = out < A + A_BYTES and A < out + BATCH * (N + 1) * WORD
        st, text, goes_on = emu.check("extract", PLAN, A, out, BATCH, 0)
        assert (st, goes_on, text) == ((EINVAL, False, SE + T_IN) if want else (OK, True, "")), off
