"""CPU stepping of the automorphism key-switch kernel (tests/emu_galoisks/emu_galoisks.cpp: polydot_galoisks_kernel stepped thread by thread
with the kernel's own headers: sigma_g of a[r][1] through the transpose image, one forward transform per term, two inverses,
sigma_g of a[r][0] through the image and added in) against the stepped explicit route (the automorphism kernel's stepping, the
two-component gadget kernel's, the addition in Python integers), against a numpy statement of sigma_g with a trivial key, against
the phase of a noise-free key with the oracle's products, and the entry point's argument list (csrc/api_checks.h:
check_galois_keyswitch), the hazard tags, the LDS banks of the two permutations and the sanitizer program, without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import emu_library
from conftest import P64, ROOT, _make, p64
from test_cmux_emu import TRIVIAL
from test_extprod_emu import input_rows
from test_gadget2_emu import EmuGadget2, pair_rows
from test_gadget_emu import MODES, POLICIES, gadget_pairs
from test_galois_emu import EmuGalois, sigma
from test_lds_banks import conflict_degree
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FN = "tn_poly_galois_keyswitch_prepared_dev"
BATCH = 7
P32 = ctypes.POINTER(ctypes.c_uint32)


def elements(n):
    """The Galois elements of the kernel tests: the identity, the two smallest generators' first powers, the last element below
    n, the first above it (every odd word negated), the conjugation 2n - 1 and one seeded."""
    seeded = int(np.random.default_rng(n).integers(0, 2 * n)) | 1
    return [1, 3, 5, n - 1, n + 1, 2 * n - 1, seeded]


class EmuGaloisKs:
    """The entry points of tests/emu_galoisks/emu_galoisks.cpp in tests/emu_galoisks/_build/libemu_galoisks.so (brought up to date
    first: nothing to do when the library is newer than its sources and headers); the shapes' threads from tests/emu's library."""

    def __init__(self):
        _make("tests/emu_galoisks")
        L = self.lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_galoisks", "_build", "libemu_galoisks.so"))
        self.emu = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_galois_keyswitch_prepared.argtypes = [u32, u64, u64, ci, P64, u32, P64, sz, P64, sz, sz, u32, u32]
        L.emu_galoisks_dst_row.argtypes = [u32, u32, P32]
        L.emu_galoisks_dst_row.restype = None
        L.emu_galoisks_api_check.argtypes = [u32, ci, ci, ci, u64, vp, u32, vp, vp, sz, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]
        self.emu.emu_galois_lpt.argtypes = [u32]; self.emu.emu_galois_lpt.restype = u32

    def status(self, n, q, psi, a, g, bhat, terms, w, balanced=False, canonical=False):
        """-> (the stepping's return code, c): 0 ok, 9 a hazard tag."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch = a.shape[0]
        assert a.shape[1:] == (2, n)
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (2 * terms, batch * 2 * terms)
        sets = 1 if bhat.shape[0] == 2 * terms else batch
        c = np.empty((batch, 2, n), dtype=np.uint64)
        rc = self.lib.emu_poly_galois_keyswitch_prepared(n, q, psi, int(canonical), p64(a), g, p64(bhat), sets, p64(c), batch, terms, w, int(balanced))
        return rc, c

    def keyswitch(self, n, q, psi, a, g, bhat, terms, w, balanced=False, canonical=False):
        """a: (batch, 2, n); bhat: (2 * terms, n) for one shared key or (batch * 2 * terms, n) -> (batch, 2, n)."""
        rc, c = self.status(n, q, psi, a, g, bhat, terms, w, balanced, canonical)
        assert rc == 0, rc
        return c

    def dst_row(self, logn, g):
        """-> (image word of every source word of a row, negated) under sigma_g: galois_core.h's galois_dst."""
        dst = np.empty(1 << logn, dtype=np.uint32)
        self.lib.emu_galoisks_dst_row(logn, g, dst.ctypes.data_as(P32))
        return (dst & np.uint32(0x7fffffff)).astype(np.int64), (dst >> np.uint32(31)).astype(bool)

    def threads(self, logn):
        return (1 << logn) >> self.emu.emu_galois_lpt(logn)

    def check(self, view, a, g, b, c, sets=1, batch=1, terms=1, base_log=1, flags=0):
        """check_galois_keyswitch on the plan view (n, elem_bytes, has_fused, omega_only, q) -> (status, text, goes on to a launch)."""
        return emu_library.api_check(self.lib.emu_galoisks_api_check, *view, a, g, b, c, sets, batch, terms, base_log, flags)


@pytest.fixture(scope="module")
def ks():
    return EmuGaloisKs()


@pytest.fixture(scope="module")
def gal():
    return EmuGalois()


@pytest.fixture(scope="module")
def gadget2():
    return EmuGadget2()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def key_rows(batch, terms, shared):
    """Rows of a case's b for the key: pair_rows ((batch, 2, terms)); a shared key is row 0's for every row."""
    idx = pair_rows(batch, terms)
    if shared:
        idx[1:] = idx[0]
    return idx


def stepped_route(gal, gadget2, n, q, psi, a, g, bh, terms, w, balanced, canonical):
    """The contract, stepped: the automorphism kernel's stepping on a viewed as batch * 2 rows, the two-component gadget kernel's
    stepping on the rotated a[r][1] rows, component 0 plus the rotated a[r][0] in Python integers."""
    batch = a.shape[0]
    rot = gal.automorphism(n, q, a.reshape(batch * 2, n), [g])[:, 0].reshape(batch, 2, n)
    want = gadget2.multidot(n, q, psi, np.ascontiguousarray(rot[:, 1]), bh, 2, terms, w, balanced, canonical)
    want[:, 0] = ((want[:, 0].astype(object) + rot[:, 0].astype(object)) % q).astype(np.uint64)
    return want


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepping_matches_the_stepped_explicit_route(ks, gal, gadget2, prep, case, canonical):
    """Batch 7 (the all-(q - 1) row and unreduced full-width rows in every launch), every (terms, w) of gadget_pairs, a shared key
    and a key per row, both digit modes, seven Galois elements: the stepped result equals the stepped explicit route."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        a7 = np.ascontiguousarray(a[input_rows(BATCH, 2, first)])        # (7, 2, n)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            for balanced in MODES:
                for g in elements(n):
                    where = (case, canonical, terms, w, shared, balanced, g)
                    c = ks.keyswitch(n, q, psi, a7, g, bh, terms, w, balanced, canonical)
                    assert np.array_equal(c, stepped_route(gal, gadget2, n, q, psi, a7, g, bh, terms, w, balanced, canonical)), where


def trivial_key(n, q, component, terms, w):
    """(2 * terms, n): [o][j] = 2^(j w) at coefficient 0 for o == component, else 0."""
    b = np.zeros((2, terms, n), dtype=np.uint64)
    for j in range(terms):
        b[component, j, 0] = (1 << (j * w)) % q
    return b.reshape(2 * terms, n)


def trivial_want(a, g, q, component):
    """What a trivial key makes of a (batch, 2, n) by the numpy statement of sigma_g in include/tinyntt.h."""
    s = sigma(a, g, q)
    want = np.zeros_like(s)
    if component == 1:
        want[:] = s
    else:
        want[:, 0] = (s[:, 0] + s[:, 1]) % np.uint64(q)         # q < 2^63: the sum fits
    return want


@pytest.mark.parametrize("case", ["P256", "P1024", "P4096_60"])
@POLICIES
def test_trivial_key_returns_sigma_of_both_components(ks, prep, case, canonical):
    """Unsigned digits that cover q recompose exactly.  K[1][j] = 2^(j w), K[0] = 0: the output is (sigma_g(a0), sigma_g(a1)).
    K[0][j] = 2^(j w), K[1] = 0: it is (sigma_g(a0) + sigma_g(a1), 0).  Nothing here passes through the project's decomposition
    or its automorphism."""
    n, q, psi, a, _ = _case_data(case)
    terms, w = TRIVIAL[q.bit_length()]
    assert terms * w >= q.bit_length() and (1 << w) < q and (terms - 1) * w < 64
    a7 = np.ascontiguousarray(a[input_rows(BATCH, 2)])
    for component in (0, 1):
        bh = prep.prepare(n, q, psi, trivial_key(n, q, component, terms, w), canonical)
        for g in elements(n):
            c = ks.keyswitch(n, q, psi, a7, g, bh, terms, w, False, canonical)
            assert np.array_equal(c, trivial_want(a7, g, q, component)), (case, canonical, component, g)


def noise_free_key(oracle, n, q, psi, s, g, terms, w, seed):
    """A key from sigma_g(s) to s without noise: K[1][j] = r_j (random), K[0][j] = 2^(j w) sigma_g(s) - r_j s, so that
    K[0][j] + K[1][j] s = 2^(j w) sigma_g(s).  -> (2 * terms, n) coefficient rows."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, q, (terms, n), dtype=np.uint64)
    rs = oracle.poly_mult(r, np.broadcast_to(s, (terms, n)).copy(), q, psi)
    sig = sigma(s, g, q)
    k0 = np.array([[(int(sig[i]) * (1 << (j * w)) - int(rs[j, i])) % q for i in range(n)] for j in range(terms)], dtype=np.uint64)
    return np.concatenate([k0, r])


@pytest.mark.parametrize("case", ["P256", "P1024"])
def test_phase_is_sigma_of_the_phase(ks, prep, oracle, case):
    """out0 + out1 s = sigma_g(a0 + a1 s), exactly, for a noise-free key from sigma_g(s) to s and unsigned digits that cover q, the
    products taken from the oracle: the direction of g (against g^-1) without passing through the explicit route."""
    n, q, psi, a, _ = _case_data(case)
    terms, w = TRIVIAL[q.bit_length()]
    rng = np.random.default_rng(n + 17)
    s = rng.integers(0, q, n, dtype=np.uint64)
    a7 = np.ascontiguousarray(a[input_rows(BATCH, 2)])
    srows = np.broadcast_to(s, (BATCH, n)).copy()
    phase = (a7[:, 0] % np.uint64(q) + oracle.poly_mult(np.ascontiguousarray(a7[:, 1]), srows, q, psi)) % np.uint64(q)
    for g in elements(n):
        bh = prep.prepare(n, q, psi, noise_free_key(oracle, n, q, psi, s, g, terms, w, g), False)
        c = ks.keyswitch(n, q, psi, a7, g, bh, terms, w, False, False)
        got = (c[:, 0] + oracle.poly_mult(np.ascontiguousarray(c[:, 1]), srows, q, psi)) % np.uint64(q)
        assert np.array_equal(got, sigma(phase, g, q)), (case, g)
        if g != 1:
            assert not np.array_equal(got, phase % np.uint64(q)), (case, g)


@pytest.mark.parametrize("case", ["P256", (256, 1152921504606830593), "P1024", "P4096_60"])
@POLICIES
def test_hazard_tags_report_none(ks, prep, case, canonical):
    """A workgroup of one wave (n = 256, 32-bit), of more (the others), the base-case shape: the stepping's tags of the three
    hazards on the image (a scatter behind a finished transform, a read-back behind its whole scatter, a transform behind the whole
    read-back) stay silent over several rows, so that one row's second permutation is followed by the next row's first."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    for g in (1, 3, 2 * n - 1):
        rc, _ = ks.status(n, q, psi, a[input_rows(3, 2)], g, bhat[pair_rows(3, 2).ravel()], 2, q.bit_length() // 2, True, canonical)
        assert rc == 0, (case, canonical, g, rc)


def permutation_degrees(ks, logn, word, g):
    """Worst conflict degree of the scatter (a ds write of `word` bytes, lanes g words apart) and of the read-back (a ds read at
    unit stride) over every wave and register of a workgroup of the shape's threads."""
    n, threads = 1 << logn, ks.threads(logn)
    dst, _ = ks.dst_row(logn, g)
    worst_w = worst_r = 1
    for r in range(n // threads):
        for wave in range(0, threads, 64):
            lanes = np.arange(wave, min(wave + 64, threads))
            src = r * threads + lanes
            worst_w = max(worst_w, conflict_degree([int(v) * word for v in dst[src]], "write", word))
            worst_r = max(worst_r, conflict_degree([int(v) * word for v in src], "read", word))
    return worst_w, worst_r


@pytest.mark.parametrize("word", [4, 8])
def test_permutations_are_bank_conflict_free_for_every_element_at_n_256(ks, word):
    for g in range(1, 512, 2):
        assert permutation_degrees(ks, 8, word, g) == (1, 1), (word, g)


def test_permutations_are_bank_conflict_free_at_the_bench_shape(ks):
    for g in elements(4096):
        assert permutation_degrees(ks, 12, 8, g) == (1, 1), g


def test_scatter_map_is_the_definition(ks):
    """galois_dst against the numpy statement: source word i goes to i g mod 2n, negated from n on."""
    for logn in (2, 8, 13):
        n = 1 << logn
        for g in elements(n) if n > 4 else (1, 3, 5, 7):
            dst, neg = ks.dst_row(logn, g)
            t = np.arange(n) * g % (2 * n)
            assert np.array_equal(dst, t % n) and np.array_equal(neg, t >= n), (n, g)
            assert len(set(dst.tolist())) == n


# ---- the argument list -------------------------------------------------------------------------
N, WORD, Q, W = 4, 4, 7681, 4                               # the smallest plan: rows of 16 bytes; 2^W < Q
ROW = N * WORD
FUSED, GENERAL, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (0, 0, 0, 0, 0)
A, B, C = 1 << 20, 1 << 30, 1 << 40
BATCH_, TERMS, G = 5, 2, 3
T_ROWS = FN + ": batch * 2 * terms too large for one call (max 2^31 - 1 digit rows)"
T_OVERLAP = FN + ": output must not alias or overlap an input"
T_FUSED = FN + ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_SETS = FN + ": bhat_sets must be 1 (one set of operands for every row) or batch"
T_BASE = FN + ": need 1 <= base_log and 2^base_log < q"
T_EVEN = FN + ": galois[0] = 4 is not an odd element below 2n"
T_BIG = FN + ": galois[0] = 9 is not an odd element below 2n"
SET = 2 * TERMS                                             # rows of one key

# (id, view, a, bhat, c, keywords, status, text or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, B, C, {}, OK, None, True),
    ("shared-ok", FUSED, A, B, C, dict(sets=1), OK, None, True),
    ("balanced-ok", FUSED, A, B, C, dict(flags=1), OK, None, True),
    ("identity-ok", FUSED, A, B, C, dict(g=1), OK, None, True),
    ("conjugation-ok", FUSED, A, B, C, dict(g=2 * N - 1), OK, None, True),
    # one row per fault, in the order of the list
    ("null-plan", NULL, A, B, C, {}, EINVAL, FN + ": plan is NULL", False),
    ("general-plan", GENERAL, A, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("galois-even", FUSED, A, B, C, dict(g=4), EINVAL, T_EVEN, False),
    ("galois-0", FUSED, A, B, C, dict(g=0), EINVAL, FN + ": galois[0] = 0 is not an odd element below 2n", False),
    ("galois-2n-plus-1", FUSED, A, B, C, dict(g=2 * N + 1), EINVAL, T_BIG, False),
    ("terms-0", FUSED, A, B, C, dict(terms=0), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2", FUSED, A, B, C, dict(flags=2), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0", FUSED, A, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("base-log-k", FUSED, A, B, C, dict(base_log=13), EINVAL, T_BASE, False),
    ("shift-64", FUSED, A, B, C, dict(terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-2^31", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 29, terms=2, base_log=1), EINVAL, T_ROWS, False),
    ("rows-2^31-one-term", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 30, terms=1), EINVAL, T_ROWS, False),
    ("rows-2^31-minus-2", FUSED, A, 1 << 50, 1 << 58, dict(sets=1, batch=2 ** 30 - 1, terms=1), OK, None, True),
    ("rows-batch-2^63", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 63, terms=1), EINVAL, T_ROWS, False),
    ("batch0-null", FUSED, None, None, None, dict(batch=0, sets=1), OK, None, False),
    ("null-a", FUSED, None, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-bhat", FUSED, A, None, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-c", FUSED, A, B, None, {}, EINVAL, FN + ": NULL buffer", False),
    ("sets-2", FUSED, A, B, C, dict(sets=2), EINVAL, T_SETS, False),
    # overlap by byte range: c's batch * 2 rows against a's batch * 2 rows ...
    ("c-is-a", FUSED, A, B, A, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-a", FUSED, A, B, A + (BATCH_ * 2 - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-last-byte-is-first-of-a", FUSED, A, B, A - BATCH_ * 2 * ROW + 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-before-a", FUSED, A, B, A - BATCH_ * 2 * ROW, {}, OK, None, True),
    ("c-over-last-byte-of-a", FUSED, A, B, A + BATCH_ * 2 * ROW - 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-a", FUSED, A, B, A + BATCH_ * 2 * ROW, {}, OK, None, True),
    # ... against a shared key's 2 * terms rows ...
    ("c-over-first-row-of-the-key", FUSED, A, B, B - (BATCH_ * 2 - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-before-the-key", FUSED, A, B, B - BATCH_ * 2 * ROW, dict(sets=1), OK, None, True),
    ("c-over-last-row-of-the-key", FUSED, A, B, B + (SET - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-past-the-key", FUSED, A, B, B + SET * ROW, dict(sets=1), OK, None, True),
    # ... and against the batch keys of a launch with a key per row
    ("c-past-the-first-key-of-the-keys", FUSED, A, B, B + SET * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-the-keys", FUSED, A, B, B + (BATCH_ * SET - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-the-keys", FUSED, A, B, B + BATCH_ * SET * ROW, {}, OK, None, True),
    # two faults: the order (plan, kernels, galois, terms, flags, base_log, shift, rows, batch 0, buffers, sets, overlap)
    ("null-plan-galois-even", NULL, A, B, C, dict(g=4), EINVAL, FN + ": plan is NULL", False),
    ("general-plan-galois-even", GENERAL, A, B, C, dict(g=4), EUNSUPPORTED, T_FUSED, False),
    ("general-plan-null-a", GENERAL, None, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("galois-even-terms-0", FUSED, A, B, C, dict(g=4, terms=0), EINVAL, T_EVEN, False),
    ("galois-even-batch-0", FUSED, None, None, None, dict(g=4, batch=0, sets=1), EINVAL, T_EVEN, False),
    ("terms-0-flag-2", FUSED, A, B, C, dict(terms=0, flags=2), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2-base-log-0", FUSED, A, B, C, dict(flags=2, base_log=0), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0-null-a", FUSED, None, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("shift-64-rows", FUSED, 4096, 4096, 4096, dict(sets=1, batch=2 ** 31, terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-null-a", FUSED, None, 4096, 4096, dict(sets=1, batch=2 ** 31), EINVAL, T_ROWS, False),
    ("batch0-sets-2", FUSED, A, B, C, dict(batch=0, sets=2), OK, None, False),
    ("null-a-sets-2", FUSED, None, B, C, dict(sets=2), EINVAL, FN + ": NULL buffer", False),
    ("sets-2-c-is-a", FUSED, A, B, A, dict(sets=2), EINVAL, T_SETS, False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(ks, row):
    _, view, a, b, c, kw, status, text, launches = row
    full = dict(g=G, sets=BATCH_, batch=BATCH_, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    g = full.pop("g")
    st, got, goes_on = ks.check(view, a, g, b, c, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got


def test_overlap_is_the_intersection_of_the_byte_ranges(ks):
    """c's batch * 2 rows against a's batch * 2 rows and against the key's sets * 2 * terms rows, every half row around them."""
    for batch in (1, 2):
        for terms in (1, 2):
            for sets in (1, batch):
                for which, in_rows in (("a", batch * 2), ("bhat", sets * 2 * terms)):
                    for off in range(-5 * ROW, (in_rows + 2) * ROW + 1, ROW // 2):
                        out = A + off
                        want = out < A + in_rows * ROW and A < out + batch * 2 * ROW
                        a, b = (A, B) if which == "a" else (B, A)
                        st, text, goes_on = ks.check(FUSED, a, G, b, out, sets=sets, batch=batch, terms=terms, base_log=W)
                        assert (st, goes_on) == ((EINVAL, False) if want else (OK, True)), (batch, terms, sets, which, off)
                        assert text == (T_OVERLAP if want else "")


def test_sanitizer_program_runs_clean():
    """The stepping's cases (tests/emu_galoisks/emu_galoisks.cpp, behind EMU_SANITIZE_CASES) under AddressSanitizer + UBSan: n = 256 at both
    lane widths and n = 4096 / 60-bit, both policies, batch 2 x 2 terms, a shared key and a key per row, both digit modes,
    g in {1, 3, n + 1, 2n - 1}, each against the stepped automorphism, the stepped pair and the addition (4 checks each: 384), and
    the argument list on made-up addresses (246).  A stand-alone program of its own (tests/emu_galoisks/sanitize_galoisks.cpp): nothing is
    loaded into Python, and sanitize_driver's family lines stay as tests/test_emu.py pins them."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_galoisks")
    b = subprocess.run(["make", "-j8", "-C", d, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-2000:]
    r = subprocess.run([os.path.join(d, "_build", "sanitize_galoisks")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    counts = {name: int(v) for name, v in re.findall(r"^(\w+): (\d+) checks$", r.stdout, re.M)}
    assert counts == {"galoisks": 630}, counts
    assert re.search(r"^sanitize_galoisks: 630 checks, 0 failures$", r.stdout, re.M), r.stdout[-500:]
