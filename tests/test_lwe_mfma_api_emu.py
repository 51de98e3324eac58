"""The argument lists of tn_lwe_ksk_prepared_bytes, tn_lwe_ksk_prepare_dev and tn_lwe_keyswitch_prepared_dev
(tiny_ntt_amd/csrc/api_checks.h: check_lwe_ksk_bytes, check_lwe_ksk_prepare, check_lwe_keyswitch_prepared, the lists capi.cpp
runs) on the CPU: one row per branch, in the order of the list, then rows with two faults that pin the order, then the overlap rule
byte by byte.  No pointer is read."""
import pytest

import lwe_mfma_cases as M
from test_lwe_api_emu import A, B, C, EINVAL, EUNSUPPORTED, GENERAL, N, NULL, OK, OMEGA, PLAN, Q, T_ANY, T_BASE, T_IN, T_NIN, T_NOUT, WIDE, WORD, words

BY, PR, KS = "tn_lwe_ksk_prepared_bytes: ", "tn_lwe_ksk_prepare_dev: ", "tn_lwe_keyswitch_prepared_dev: "
T_BYTE = ("digits wider than a signed byte are not supported (unsigned base_log <= 7, TN_GADGET_BALANCED base_log <= 8): "
          "tn_lwe_keyswitch_dev is the route")
T_ALIGN = "kprep must be aligned to 16 bytes"
T_T64 = "terms must be at most 64"
BATCH, NIN, NOUT, TERMS, W = 3, 8, 5, 2, 4
LWE_BYTES, OUT_BYTES, KSK_BYTES = BATCH * (NIN + 1) * WORD, BATCH * (NOUT + 1) * WORD, NIN * TERMS * (NOUT + 1) * WORD
KPREP_BYTES = M.prepared_bytes(Q, NIN, NOUT, TERMS)          # q = 7681: 2 limbs, one K step, one column tile: 2 KiB


@pytest.fixture(scope="module")
def emu():
    return M.emu_lwe_mfma()


def test_the_view_s_prepared_key(emu):
    assert KPREP_BYTES == 2048 == emu.bytes(Q, NIN, NOUT, TERMS) and KPREP_BYTES % 16 == 0


# (id, view, keywords, bytes pointer, status, text, goes on)
BYTES = [
    ("ok", PLAN, {}, A, OK, "", True),
    ("general-plan-ok", GENERAL, {}, A, OK, "", True),
    ("omega-plan-ok", OMEGA, {}, A, OK, "", True),
    ("dims-max-ok", PLAN, dict(n_in=65536, n_out=65536, terms=3), A, OK, "", True),
    ("2^22-slots-ok", PLAN, dict(n_in=65536, terms=64), A, OK, "", True),
    ("null-plan", NULL, {}, A, EINVAL, BY + "plan is NULL", False),
    ("n-in-0", PLAN, dict(n_in=0), A, EINVAL, BY + T_NIN, False),
    ("n-in-above", PLAN, dict(n_in=65537), A, EINVAL, BY + T_NIN, False),
    ("n-out-0", PLAN, dict(n_out=0), A, EINVAL, BY + T_NOUT, False),
    ("n-out-above", PLAN, dict(n_out=65537), A, EINVAL, BY + T_NOUT, False),
    ("terms-0", PLAN, dict(terms=0), A, EINVAL, BY + "terms must be at least 1", False),
    ("terms-65", PLAN, dict(terms=65), A, EINVAL, BY + T_T64, False),
    ("null-bytes", PLAN, {}, None, EINVAL, BY + "NULL argument", False),
    # two faults: the order (plan, n_in, n_out, terms, answer)
    ("null-plan-n-in-0", NULL, dict(n_in=0), A, EINVAL, BY + "plan is NULL", False),
    ("n-in-0-n-out-0", PLAN, dict(n_in=0, n_out=0), A, EINVAL, BY + T_NIN, False),
    ("n-out-0-terms-0", PLAN, dict(n_out=0, terms=0), A, EINVAL, BY + T_NOUT, False),
    ("terms-65-null-bytes", PLAN, dict(terms=65), None, EINVAL, BY + T_T64, False),
]


@pytest.mark.parametrize("row", BYTES, ids=[r[0] for r in BYTES])
def test_prepared_bytes_argument_list(emu, row):
    _, view, kw, ptr, status, text, goes_on = row
    full = dict(n_in=NIN, n_out=NOUT, terms=TERMS)
    full.update(kw)
    st, got, on = emu.check("bytes", view, full["n_in"], full["n_out"], full["terms"], ptr)
    assert (st, on, got) == (status, goes_on, text)


# (id, view, ksk, kprep, keywords, status, text, launches)
PREPARE = [
    ("ok", PLAN, A, B, {}, OK, "", True),
    ("general-plan-ok", GENERAL, A, B, {}, OK, "", True),
    ("omega-plan-ok", OMEGA, A, B, {}, OK, "", True),
    ("wide-ok", WIDE, A, B, {}, OK, "", True),
    ("null-plan", NULL, A, B, {}, EINVAL, PR + "plan is NULL", False),
    ("n-in-0", PLAN, A, B, dict(n_in=0), EINVAL, PR + T_NIN, False),
    ("n-out-above", PLAN, A, B, dict(n_out=65537), EINVAL, PR + T_NOUT, False),
    ("terms-0", PLAN, A, B, dict(terms=0), EINVAL, PR + "terms must be at least 1", False),
    ("terms-65", PLAN, A, B, dict(terms=65), EINVAL, PR + T_T64, False),
    ("null-ksk", PLAN, None, B, {}, EINVAL, PR + "NULL buffer", False),
    ("null-kprep", PLAN, A, None, {}, EINVAL, PR + "NULL buffer", False),
    ("kprep-off-by-8", PLAN, A, B + 8, {}, EINVAL, PR + T_ALIGN, False),
    ("kprep-off-by-1", PLAN, A, B + 1, {}, EINVAL, PR + T_ALIGN, False),
    ("kprep-is-ksk", PLAN, A, A, {}, EINVAL, PR + T_IN, False),
    ("kprep-over-last-word-of-ksk", PLAN, A, A + KSK_BYTES - 16, {}, EINVAL, PR + T_IN, False),
    ("kprep-just-past-ksk", PLAN, A, A + KSK_BYTES, {}, OK, "", True),
    ("kprep-just-before-ksk", PLAN, A, A - KPREP_BYTES, {}, OK, "", True),
    ("kprep-last-word-is-first-of-ksk", PLAN, A, A - KPREP_BYTES + 16, {}, EINVAL, PR + T_IN, False),
    # two faults: the order (plan, n_in, n_out, terms, buffers, alignment, overlap)
    ("terms-0-null", PLAN, None, None, dict(terms=0), EINVAL, PR + "terms must be at least 1", False),
    ("null-before-alignment", PLAN, None, B + 8, {}, EINVAL, PR + "NULL buffer", False),
    ("alignment-before-overlap", PLAN, A, A + 8, {}, EINVAL, PR + T_ALIGN, False),
]


@pytest.mark.parametrize("row", PREPARE, ids=[r[0] for r in PREPARE])
def test_prepare_argument_list(emu, row):
    _, view, ksk, kprep, kw, status, text, launches = row
    full = dict(n_in=NIN, n_out=NOUT, terms=TERMS)
    full.update(kw)
    st, got, goes_on = emu.check("prepare", view, ksk, kprep, full["n_in"], full["n_out"], full["terms"])
    assert (st, goes_on, got) == (status, launches, text)


# (id, view, lwe, kprep, out, keywords, status, text, launches)
KEYSWITCH = [
    ("ok", PLAN, A, B, C, {}, OK, "", True),
    ("balanced-ok", PLAN, A, B, C, dict(flags=1), OK, "", True),
    ("general-plan-ok", GENERAL, A, B, C, {}, OK, "", True),
    ("omega-plan-ok", OMEGA, A, B, C, {}, OK, "", True),
    ("dims-1-ok", PLAN, A, B, C, dict(n_in=1, n_out=1), OK, "", True),
    ("unsigned-7-ok", PLAN, A, B, C, dict(base_log=7), OK, "", True),
    ("balanced-8-ok", PLAN, A, B, C, dict(base_log=8, flags=1), OK, "", True),
    ("2^22-slots-ok", PLAN, A, B, 1 << 50, dict(n_in=65536, terms=64, base_log=1), OK, "", True),
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
    ("shift-64", PLAN, A, B, C, dict(terms=65, base_log=1), EINVAL, KS + "(terms - 1) * base_log must be below 64", False),
    ("unsigned-8", PLAN, A, B, C, dict(base_log=8), EUNSUPPORTED, KS + T_BYTE, False),
    ("balanced-9", PLAN, A, B, C, dict(base_log=9, flags=1), EUNSUPPORTED, KS + T_BYTE, False),
    ("wide-32", WIDE, A, B, C, dict(base_log=32), EUNSUPPORTED, KS + T_BYTE, False),
    ("lwe-words-2^31", PLAN, A, B, C, dict(batch=2 ** 28), EINVAL, KS + words("n_in"), False),
    ("out-words-2^31", PLAN, A, B, C, dict(batch=2 ** 28, n_in=1, n_out=7), EINVAL, KS + words("n_out"), False),
    ("batch0-null", PLAN, None, None, None, dict(batch=0), OK, "", False),
    ("null-lwe", PLAN, None, B, C, {}, EINVAL, KS + "NULL buffer", False),
    ("null-kprep", PLAN, A, None, C, {}, EINVAL, KS + "NULL buffer", False),
    ("null-out", PLAN, A, B, None, {}, EINVAL, KS + "NULL buffer", False),
    ("kprep-off-by-4", PLAN, A, B + 4, C, {}, EINVAL, KS + T_ALIGN, False),
    ("out-is-lwe", PLAN, A, B, A, {}, EINVAL, KS + T_ANY, False),
    ("out-over-last-byte-of-lwe", PLAN, A, B, A + LWE_BYTES - 1, {}, EINVAL, KS + T_ANY, False),
    ("out-just-past-lwe", PLAN, A, B, A + LWE_BYTES, {}, OK, "", True),
    ("out-just-before-lwe", PLAN, A, B, A - OUT_BYTES, {}, OK, "", True),
    ("out-is-kprep", PLAN, A, B, B, {}, EINVAL, KS + T_ANY, False),
    ("out-over-last-byte-of-kprep", PLAN, A, B, B + KPREP_BYTES - 1, {}, EINVAL, KS + T_ANY, False),
    ("out-in-the-padding-of-kprep", PLAN, A, B, B + KPREP_BYTES - OUT_BYTES, {}, EINVAL, KS + T_ANY, False),
    ("out-just-past-kprep", PLAN, A, B, B + KPREP_BYTES, {}, OK, "", True),
    ("out-just-before-kprep", PLAN, A, B, B - OUT_BYTES, {}, OK, "", True),
    # two faults: the order (plan, n_in, n_out, terms, flags, base_log, shift, key rows, byte digits, words of lwe, of out, batch 0,
    # buffers, alignment, overlap)
    ("null-plan-n-in-0", NULL, A, B, C, dict(n_in=0), EINVAL, KS + "plan is NULL", False),
    ("flag-2-unsigned-8", PLAN, A, B, C, dict(flags=2, base_log=8), EINVAL, KS + "unknown flag bit", False),
    ("base-log-before-byte-digits", PLAN, A, B, C, dict(base_log=13), EINVAL, KS + T_BASE, False),
    ("shift-before-byte-digits", WIDE, A, B, C, dict(base_log=33, terms=3), EINVAL, KS + "(terms - 1) * base_log must be below 64", False),
    ("byte-digits-before-words", PLAN, A, B, C, dict(base_log=8, batch=2 ** 31), EUNSUPPORTED, KS + T_BYTE, False),
    ("byte-digits-before-batch-0", PLAN, None, None, None, dict(base_log=8, batch=0), EUNSUPPORTED, KS + T_BYTE, False),
    ("words-null", PLAN, None, None, None, dict(batch=2 ** 31), EINVAL, KS + words("n_in"), False),
    ("batch0-misaligned-overlap", PLAN, A, B + 4, A, dict(batch=0), OK, "", False),
    ("null-before-alignment", PLAN, None, B + 4, C, {}, EINVAL, KS + "NULL buffer", False),
    ("alignment-before-overlap", PLAN, A, B + 4, A, {}, EINVAL, KS + T_ALIGN, False),
]


@pytest.mark.parametrize("row", KEYSWITCH, ids=[r[0] for r in KEYSWITCH])
def test_keyswitch_prepared_argument_list(emu, row):
    _, view, lwe, kprep, out, kw, status, text, launches = row
    full = dict(batch=BATCH, n_in=NIN, n_out=NOUT, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    st, got, goes_on = emu.check("keyswitch", view, lwe, kprep, out, full["batch"], full["n_in"], full["n_out"], full["terms"], full["base_log"],
                                 full["flags"])
    assert (st, goes_on, got) == (status, launches, text)


def test_sum_bound_stands_behind_the_dimensions(emu):
    """n_in * terms above 2^22 is unreachable with today's limits (2^16, 64 terms), as in tn_lwe_keyswitch_dev: the largest call passes."""
    assert emu.check("keyswitch", PLAN, A, B, 1 << 50, 3, 65536, 5, 64, 1, 0)[0] == OK
    assert emu.check("prepare", PLAN, A, 1 << 50, 65536, 5, 64)[0] == OK


def test_overlap_is_the_intersection_of_the_byte_ranges(emu):
    """Every word around the inputs: out against lwe and against kprep (its padding included), kprep against ksk."""
    for off in range(-2 * LWE_BYTES, KPREP_BYTES + 2 * LWE_BYTES, 4):
        out = A + off
        want = out < A + LWE_BYTES and A < out + OUT_BYTES
        st, text, goes_on = emu.check("keyswitch", PLAN, A, B, out, BATCH, NIN, NOUT, TERMS, W, 0)
        assert (st, goes_on, text) == ((EINVAL, False, KS + T_ANY) if want else (OK, True, "")), off
        want = out < A + KPREP_BYTES and A < out + OUT_BYTES
        st, text, goes_on = emu.check("keyswitch", PLAN, B, A, out, BATCH, NIN, NOUT, TERMS, W, 0)
        assert (st, goes_on, text) == ((EINVAL, False, KS + T_ANY) if want else (OK, True, "")), off
    for off in range(-KPREP_BYTES - 64, KSK_BYTES + 64, 16):
        kprep = A + off
        want = kprep < A + KSK_BYTES and A < kprep + KPREP_BYTES
        st, text, goes_on = emu.check("prepare", PLAN, A, kprep, NIN, NOUT, TERMS)
        assert (st, goes_on, text) == ((EINVAL, False, PR + T_IN) if want else (OK, True, "")), off
