"""CPU stepping of the automorphism kernels (tests/emu/emu_galois.cpp: automorphism_kernel and automorphism_hat_kernel
stepped tile by tile with the header the gfx950 kernels are compiled from, csrc/galois_core.h) against sigma_g written from its
definition (include/tinyntt.h) in numpy below, the index maps' properties, the LDS bank model of the gathers, the argument list of
both entry points (csrc/api_checks.h: check_automorphism) and numtheory.galois_element, without a GPU."""
import ctypes
import functools

import numpy as np
import pytest

import emu_library
from conftest import P64, PARAMS, ntt_prime_below, p64
from test_hat_emu import EmuHat
from test_prepared_emu import Q23, Q60, EmuPrepared, shape_params
from tiny_ntt_amd import numtheory

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
P32 = ctypes.POINTER(ctypes.c_uint32)
GALOIS_MAX = 16


# ---- the oracle: sigma_g from the definition, explicit indices, nothing of the code under test ----------------------
def sigma(a, g, q):
    """out[t] = a[i] mod q for t = i g mod 2n < n, out[t - n] = (q - a[i] mod q) mod q otherwise; a: (..., n) unsigned words."""
    a = np.asarray(a, dtype=np.uint64)
    n = a.shape[-1]
    assert g % 2 == 1 and 1 <= g < 2 * n
    x = a % np.uint64(q)
    out = np.empty_like(x)
    i = np.arange(n)
    t = i * g % (2 * n)
    low = t < n
    out[..., t[low]] = x[..., i[low]]
    out[..., t[~low] - n] = (np.uint64(q) - x[..., i[~low]]) % np.uint64(q)
    return out


def named_elements(n):
    return [1, 3, 5, n - 1, n + 1, 2 * n - 1]


def seeded_elements(n, count, seed):
    rng = np.random.default_rng(seed)
    return [int(v) | 1 for v in rng.integers(0, 2 * n, count)]


# ---- the library ------------------------------------------------------------------------------------------------
def u32s(values):
    return (ctypes.c_uint32 * max(len(values), 1))(*values)


class EmuGalois:
    """The entry points of tests/emu/emu_galois.cpp in tests/emu/_build/libemu.so."""

    def __init__(self):
        L = self.lib = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_automorphism.argtypes = [u32, u64, P64, P64, sz, P32, sz]
        L.emu_automorphism_prepared.argtypes = [u32, u64, u64, ci, P64, P64, sz, P32, sz, ctypes.POINTER(ci)]
        L.emu_galois_src_row.argtypes = [u32, u32, P32]
        L.emu_galois_hat_src_row.argtypes = [u32, u32, ci, u32, P32, P32]
        L.emu_galois_lpt.argtypes = [u32]; L.emu_galois_lpt.restype = u32
        L.emu_galois_tile_rows.argtypes = [u32]; L.emu_galois_tile_rows.restype = u32
        L.emu_galois_api_check.argtypes = [u32, ci, ci, ci, u64, ci, vp, vp, sz, P32, sz, ctypes.POINTER(ci), ctypes.c_char_p, sz]

    def automorphism(self, n, q, a, galois):
        """a: (batch, n) -> (batch, count, n)"""
        a = np.atleast_2d(np.ascontiguousarray(a, dtype=np.uint64))
        out = np.empty((a.shape[0], len(galois), n), dtype=np.uint64)
        rc = self.lib.emu_automorphism(n, q, p64(a), p64(out), a.shape[0], u32s(galois), len(galois))
        assert rc == 0, rc
        return out

    def automorphism_prepared(self, n, q, psi, xhat, galois, canonical=False):
        """xhat: (rows, n) prepared rows -> ((rows, count, n), the rows are in the base-case format)"""
        xhat = np.atleast_2d(np.ascontiguousarray(xhat, dtype=np.uint64))
        out = np.empty((xhat.shape[0], len(galois), n), dtype=np.uint64)
        bc = ctypes.c_int(-1)
        rc = self.lib.emu_automorphism_prepared(n, q, psi, int(canonical), p64(xhat), p64(out), xhat.shape[0], u32s(galois), len(galois), ctypes.byref(bc))
        assert rc == 0, rc
        return out, bool(bc.value)

    def src_row(self, logn, g):
        """(source index, negated) of every destination of the coefficient map"""
        out = np.empty(1 << logn, dtype=np.uint32)
        self.lib.emu_galois_src_row(logn, g, out.ctypes.data_as(P32))
        return out & np.uint32(0x7FFFFFFF), (out >> np.uint32(31)).astype(bool)

    def hat_src_row(self, logn, lpt, bc, g):
        """(source word, exponent of psi of the base case's factor) of every destination word of the prepared map"""
        src, fexp = np.empty(1 << logn, dtype=np.uint32), np.empty(1 << logn, dtype=np.uint32)
        self.lib.emu_galois_hat_src_row(logn, lpt, int(bc), g, src.ctypes.data_as(P32), fexp.ctypes.data_as(P32))
        return src, fexp

    def check(self, view, prepared, a, out, batch, galois, count=None):
        """check_automorphism on the plan view (n, elem_bytes, has_fused, omega_only, q) -> (status, text, goes on to a launch)."""
        g = None if galois is None else u32s(galois)
        count = len(galois) if count is None else count
        return emu_library.api_check(self.lib.emu_galois_api_check, *view, int(prepared), a, out, batch, g, count)


@pytest.fixture(scope="module")
def gal():
    return EmuGalois()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


@pytest.fixture(scope="module")
def hat():
    return EmuHat()


# ---- coefficient stepping equals the definition ------------------------------------------------------------------------
COEFF_N = [4, 8, 64, 256, 1024, 4096, 8192]


def coefficient_rows(n, q, batch, seed):
    """Random full-width words; a row of zeros and a row cycling through q, 2q, q - 1, the all-ones word and 0 (in row 0's
    first half when there is one row only)."""
    rng = np.random.default_rng(seed)
    word = 2 ** 32 - 1 if q < 2 ** 31 else 2 ** 64 - 1
    a = rng.integers(0, word, (batch, n), dtype=np.uint64, endpoint=True)
    special = np.resize(np.array([q, 2 * q, q - 1, word, 0], dtype=np.uint64), n)
    if batch >= 3:
        a[1] = 0
        a[2] = special
    else:
        a[0, : n // 2] = special[: n // 2]
    return a


@pytest.mark.parametrize("wide", [False, True], ids=["32-bit", "64-bit"])
@pytest.mark.parametrize("n", COEFF_N)
def test_coefficient_stepping_equals_the_definition(gal, n, wide):
    """Every named element and 16 seeded ones one by one, three in one call with a repeated element, sixteen in one call with a
    repeated element; batches 1, 3 and one that ends inside a tile; outputs canonical (never q)."""
    q = Q60 if wide else (Q23 if n <= 4096 else 7681)
    logn = n.bit_length() - 1
    rpp = gal.lib.emu_galois_tile_rows(logn)
    assert rpp == max(1, 1024 // n)
    elements = named_elements(n) + seeded_elements(n, 16, n + wide)
    for batch in (1, 3, 2 * rpp + 1 if rpp > 1 else 2):
        a = coefficient_rows(n, q, batch, 7 * n + batch)
        ref = {g: sigma(a, g, q) for g in set(elements)}
        for g in elements:
            got = gal.automorphism(n, q, a, [g])
            assert got.shape == (batch, 1, n)
            assert np.array_equal(got[:, 0], ref[g]), (n, q, batch, g)
            assert got.max() < q
        three = [elements[1], elements[5], elements[1]]
        sixteen = elements[6:21] + [elements[6]]
        for lst in (three, sixteen):
            got = gal.automorphism(n, q, a, lst)
            for m, g in enumerate(lst):
                assert np.array_equal(got[:, m], ref[g]), (n, q, batch, lst, m)


# ---- prepared stepping, every fused shape family -----------------------------------------------------------------------
HAT_CASES = ["P256", (256, Q60), (512, Q23), (512, Q60), "P1024", (1024, Q60), (2048, Q23), (2048, Q60), "P4096", "P4096_60",
             (8192, ntt_prime_below(2 ** 31, 8192)), "P8192_60"]
HAT_IDS = [c if isinstance(c, str) else f"n{c[0]}_q{c[1].bit_length()}" for c in HAT_CASES]
POLICIES = pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])


@functools.lru_cache(maxsize=None)
def hat_rows(case):
    n, q, psi = shape_params(case)
    rng = np.random.default_rng(n + q % 997)
    word = 2 ** 32 - 1 if q < 2 ** 31 else 2 ** 64 - 1
    x = rng.integers(0, word, (3, n), dtype=np.uint64, endpoint=True)
    x[1] = q - 1
    x[2] = 0; x[2, 1] = 1                     # x^1
    x.setflags(write=False)
    return n, q, psi, x


@pytest.mark.parametrize("case", HAT_CASES, ids=HAT_IDS)
@POLICIES
def test_prepared_stepping_is_the_prepared_form_of_sigma(gal, prep, hat, case, canonical):
    """galois_hat(prepare(x), g) == prepare(sigma_g(x)) word for word and unprepare of it == sigma_g(x), for the named elements
    and two seeded ones; three elements in one call equal three single calls.  n = 4096 / 60-bit runs the base-case form as
    created and the complete form under the canonical policy."""
    n, q, psi, x = hat_rows(case)
    xhat = prep.prepare(n, q, psi, x, canonical)
    elements = named_elements(n) + seeded_elements(n, 2, n)
    singles = {}
    for g in elements:
        want = sigma(x, g, q)
        got, bc = gal.automorphism_prepared(n, q, psi, xhat, [g], canonical)
        assert bc == (case == "P4096_60" and not canonical)
        singles[g] = got[:, 0]
        assert np.array_equal(got[:, 0], prep.prepare(n, q, psi, want, canonical)), (case, canonical, g)
        assert np.array_equal(hat.unprepare(n, q, psi, got[:, 0], canonical), want), (case, canonical, g)
    lst = [elements[1], elements[6], elements[1]]
    got, _ = gal.automorphism_prepared(n, q, psi, xhat, lst, canonical)
    for m, g in enumerate(lst):
        assert np.array_equal(got[:, m], singles[g]), (case, canonical, m)


@pytest.mark.parametrize("case", ["P256", "P1024", "P4096", "P8192_60"])
def test_prepared_layout_slot_j_holds_the_value_at_psi_to_the_2_brv_j_plus_1(gal, prep, case):
    """What the prepared map rests on: prepare(x^1) has psi^(2 brv(j) + 1) at slot j = (tau << LPT) | r, word (r << (logn - LPT)) | tau,
    for plans whose transform is complete."""
    n, q, psi = shape_params(case)
    logn = n.bit_length() - 1
    lpt = gal.lib.emu_galois_lpt(logn)
    x = np.zeros((1, n), dtype=np.uint64); x[0, 1] = 1
    xhat = prep.prepare(n, q, psi, x)[0]
    for j in range(n):
        word = ((j & ((1 << lpt) - 1)) << (logn - lpt)) | (j >> lpt)
        assert int(xhat[word]) == pow(psi, 2 * numtheory.bit_reverse(j, logn) + 1, q), (case, j)


# ---- map properties ----------------------------------------------------------------------------------------------------
def elements_to_check(n, seed):
    """every odd g for n <= 1024; the six named and 64 seeded ones above"""
    return list(range(1, 2 * n, 2)) if n <= 1024 else named_elements(n) + seeded_elements(n, 64, seed)


@pytest.mark.parametrize("n", COEFF_N)
def test_coefficient_source_map_is_a_signed_bijection_and_the_definition(gal, n):
    logn = n.bit_length() - 1
    i = np.arange(n, dtype=np.int64)
    for g in elements_to_check(n, n):
        src, neg = gal.src_row(logn, g)
        assert np.array_equal(np.sort(src), i), (n, g)
        t = src.astype(np.int64) * g % (2 * n)                          # where the definition sends source i
        assert np.array_equal(np.where(t < n, t, t - n), i) and np.array_equal(t >= n, neg), (n, g)


@pytest.mark.parametrize("logn", [8, 9, 10, 11, 12, 13])
def test_prepared_source_map_is_a_bijection_for_every_fused_shape(gal, logn):
    """... in the complete form of every fused (logn, LPT) and the base-case form (logn = 12): the latter keeps the parity of
    the slot, and its factor exponents compose: e_i (g - 1) for even slots is 0."""
    n = 1 << logn
    lpt = gal.lib.emu_galois_lpt(logn)
    assert lpt == (2 if logn == 8 else 3)
    words = np.arange(n)
    for bc in ([False, True] if logn == 12 else [False]):
        for g in elements_to_check(n, logn):
            src, fexp = gal.hat_src_row(logn, lpt, bc, g)
            assert np.array_equal(np.sort(src), words), (logn, bc, g)
            if bc:
                odd = ((words >> (logn - lpt)) & 1).astype(bool)          # slot parity = low bit of the register index
                assert np.array_equal(((src >> (logn - lpt)) & 1).astype(bool), odd)
                assert not fexp[~odd].any() and (fexp < 2 * n).all()
        src, fexp = gal.hat_src_row(logn, lpt, bc, 1)
        assert np.array_equal(src, words) and not fexp.any()


@pytest.mark.parametrize("wide", [False, True], ids=["32-bit", "64-bit"])
@pytest.mark.parametrize("n", COEFF_N)
def test_group_law_on_words(gal, n, wide):
    """sigma_g . sigma_h = sigma_{g h mod 2n}, sigma_1 = canonicalisation, sigma_g . sigma_{g^-1} = canonicalisation."""
    q = Q60 if wide else (Q23 if n <= 4096 else 7681)
    a = coefficient_rows(n, q, 3, n)
    canon = a % np.uint64(q)
    assert np.array_equal(gal.automorphism(n, q, a, [1])[:, 0], canon)
    h = seeded_elements(n, 1, 5 * n)[0]
    ah = gal.automorphism(n, q, a, [h])[:, 0]
    elements = elements_to_check(n, 3 * n)
    for k in range(0, len(elements), GALOIS_MAX):
        chunk = elements[k:k + GALOIS_MAX]
        composed = gal.automorphism(n, q, ah, chunk)                      # sigma_g(sigma_h(a))
        direct = gal.automorphism(n, q, a, [g * h % (2 * n) for g in chunk])
        assert np.array_equal(composed, direct), (n, chunk)
        fwd = gal.automorphism(n, q, a, chunk)
        for m, g in enumerate(chunk):
            back = gal.automorphism(n, q, fwd[:, m], [pow(g, -1, 2 * n)])[:, 0]
            assert np.array_equal(back, canon), (n, g)


@pytest.mark.parametrize("case", ["P256", "P4096_60"])
def test_group_law_on_prepared_words(gal, prep, case):
    n, q, psi, x = hat_rows(case)
    xhat = prep.prepare(n, q, psi, x)
    g, h = seeded_elements(n, 2, 11)
    gh, _ = gal.automorphism_prepared(n, q, psi, gal.automorphism_prepared(n, q, psi, xhat, [h])[0][:, 0], [g])
    direct, _ = gal.automorphism_prepared(n, q, psi, xhat, [g * h % (2 * n)])
    assert np.array_equal(gh, direct)
    back, _ = gal.automorphism_prepared(n, q, psi, gal.automorphism_prepared(n, q, psi, xhat, [g])[0][:, 0], [pow(g, -1, 2 * n)])
    assert np.array_equal(back[:, 0], xhat)


@pytest.mark.parametrize("case", ["P256", "P4096_60"])
def test_ring_homomorphism(gal, oracle, case):
    """sigma_g(a b) = sigma_g(a) sigma_g(b), the products from the oracle library."""
    n, q, psi = PARAMS[case]
    rng = np.random.default_rng(n)
    a, b = rng.integers(0, q, (2, 2, n), dtype=np.uint64)
    ab = oracle.poly_mult(a, b, q, psi)
    for g in named_elements(n)[1:] + seeded_elements(n, 2, 13):
        sa, sb, sab = (gal.automorphism(n, q, v, [g])[:, 0] for v in (a, b, ab))
        assert np.array_equal(oracle.poly_mult(sa, sb, q, psi), sab), (case, g)
        assert np.array_equal(sab, sigma(ab, g, q))


# ---- LDS banks of the gathers ---------------------------------------------------------------------------------------
def worst_bank_multiplicity(words, word_bytes):
    """Distinct addresses per bank and group of 32 lanes, the worst over the wave's two groups, for one element-wide LDS read of
    64 lanes at the word indices `words` of an image that starts on a bank boundary.  The bank of a dword at byte address a is
    (a / 4) mod 32 for a 32-bit read and (a / 4) mod 64 for a 64-bit read, whose word covers two banks.  1 is conflict free."""
    banks_of_access = {4: 32, 8: 64}[word_bytes]
    worst = 0
    for grp in (words[:32], words[32:]):
        banks = {}
        for w in set(int(v) for v in grp):
            for dword in range(word_bytes // 4):
                banks.setdefault((w * word_bytes // 4 + dword) % banks_of_access, set()).add(w)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def test_bank_model_on_strides():
    """Unit stride is free; a stride of 2 words is 2-way, of 16 words 16-way, of 32 words 32-way, for either word size (a 64-bit
    word covers two of 64 banks, a 32-bit word one of 32: words 32 apart meet in both)."""
    for word_bytes in (4, 8):
        for stride, ways in ((1, 1), (3, 1), (2, 2), (16, 16), (32, 32)):
            assert worst_bank_multiplicity([stride * i for i in range(64)], word_bytes) == ways, (word_bytes, stride)


@pytest.mark.parametrize("n", [64, 256, 1024, 4096, 8192])
def test_gather_reads_of_the_unpadded_image_are_bank_conflict_free(gal, n):
    """Consecutive lanes take consecutive destination words.  Coefficient kernel: sources at the odd stride g^-1.  Prepared
    kernel: a bit-reversal pattern; 32 consecutive destinations read 32 consecutive image words in a permuted order, a
    register block apart at most.  Every wave of a row, both word sizes, the named elements and eight seeded ones."""
    logn = n.bit_length() - 1
    for g in named_elements(n) + seeded_elements(n, 8, n):
        src, _ = gal.src_row(logn, g)
        for w0 in range(0, n, 64):
            assert worst_bank_multiplicity(src[w0:w0 + 64], 8) == 1 and worst_bank_multiplicity(src[w0:w0 + 64], 4) == 1, (n, g, w0)
        if logn >= 8:
            lpt = gal.lib.emu_galois_lpt(logn)
            for bc in ([False, True] if logn == 12 else [False]):
                hsrc, _ = gal.hat_src_row(logn, lpt, bc, g)
                for w0 in range(0, n, 64):
                    assert worst_bank_multiplicity(hsrc[w0:w0 + 64], 8) == 1 and worst_bank_multiplicity(hsrc[w0:w0 + 64], 4) == 1, (n, bc, g, w0)


# ---- the argument list -------------------------------------------------------------------------------------------------
N, WORD, Q = 4, 4, 7681                                      # the smallest plan: rows of 16 bytes, 2n = 8
ROW = N * WORD
FUSED, GENERAL, OMEGA, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (N, WORD, 0, 1, Q), (0, 0, 0, 0, 0)
A, C = 1 << 20, 1 << 40
BATCH, G3 = 5, [3, 5, 7]
COEFF, PREP = "tn_automorphism_dev", "tn_automorphism_prepared_dev"
T_FUSED = ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_COUNT = ": count must be between 1 and TN_GALOIS_MAX (16)"
T_ROWS = ": batch * count too large for one call (max 2^31 - 1 output rows)"
T_OVERLAP = ": output must not alias or overlap the input"

# (id, view, in, out, batch, galois, count or None, status, text without the name or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, C, BATCH, G3, None, OK, None, True),
    ("count-16-ok", FUSED, A, C, BATCH, [1] * 16, None, OK, None, True),
    ("null-plan", NULL, A, C, BATCH, G3, None, EINVAL, ": plan is NULL", False),
    ("count-0", FUSED, A, C, BATCH, G3, 0, EINVAL, T_COUNT, False),
    ("count-17", FUSED, A, C, BATCH, [1] * 17, None, EINVAL, T_COUNT, False),
    ("g-even", FUSED, A, C, BATCH, [3, 4, 7], None, EINVAL, ": galois[1] = 4 is not an odd element below 2n", False),
    ("g-2n", FUSED, A, C, BATCH, [3, 5, 8], None, EINVAL, ": galois[2] = 8 is not an odd element below 2n", False),
    ("g-2n-plus-1", FUSED, A, C, BATCH, [9], None, EINVAL, ": galois[0] = 9 is not an odd element below 2n", False),
    ("g-0", FUSED, A, C, BATCH, [0], None, EINVAL, ": galois[0] = 0 is not an odd element below 2n", False),
    ("rows-2^31-minus-1", FUSED, A, 1 << 50, 2 ** 31 - 1, [3], None, OK, None, True),
    ("rows-2^31", FUSED, 4096, 4096, 2 ** 31, [3], None, EINVAL, T_ROWS, False),
    ("rows-2^31-by-count", FUSED, 4096, 4096, 2 ** 29, [1, 3, 5, 7], None, EINVAL, T_ROWS, False),
    ("rows-2^31-minus-2-by-count", FUSED, A, 1 << 50, 2 ** 30 - 1, [1, 3], None, OK, None, True),
    ("rows-batch-2^63", FUSED, 4096, 4096, 2 ** 63, [1, 3], None, EINVAL, T_ROWS, False),
    ("batch0", FUSED, A, C, 0, G3, None, OK, None, False),
    ("batch0-null", FUSED, None, None, 0, None, 3, OK, None, False),
    ("null-in", FUSED, None, C, BATCH, G3, None, EINVAL, ": NULL buffer", False),
    ("null-out", FUSED, A, None, BATCH, G3, None, EINVAL, ": NULL buffer", False),
    ("null-galois", FUSED, A, C, BATCH, None, 3, EINVAL, ": NULL buffer", False),
    ("in-place", FUSED, A, A, BATCH, [3], None, EINVAL, T_OVERLAP, False),
    ("out-over-last-row-of-in", FUSED, A, A + (BATCH - 1) * ROW, BATCH, G3, None, EINVAL, T_OVERLAP, False),
    ("out-last-row-is-first-of-in", FUSED, A, A - (BATCH * 3 - 1) * ROW, BATCH, G3, None, EINVAL, T_OVERLAP, False),
    ("out-just-before-in", FUSED, A, A - BATCH * 3 * ROW, BATCH, G3, None, OK, None, True),
    ("out-just-past-in", FUSED, A, A + BATCH * ROW, BATCH, G3, None, OK, None, True),
    # two faults: the list's order (plan, fused kernels, count, elements, rows, batch 0, buffers, overlap)
    ("count-0-g-even", FUSED, A, C, BATCH, [4], 0, EINVAL, T_COUNT, False),
    ("g-even-rows", FUSED, 4096, 4096, 2 ** 31, [4], None, EINVAL, ": galois[0] = 4 is not an odd element below 2n", False),
    ("g-even-batch0", FUSED, A, C, 0, [4], None, EINVAL, ": galois[0] = 4 is not an odd element below 2n", False),
    ("rows-null-in", FUSED, None, 4096, 2 ** 31, [3], None, EINVAL, T_ROWS, False),
    ("batch0-in-place", FUSED, A, A, 0, G3, None, OK, None, False),
    ("null-in-in-place", FUSED, None, None, BATCH, G3, None, EINVAL, ": NULL buffer", False),
]


@pytest.mark.parametrize("prepared", [False, True], ids=["coefficients", "prepared"])
@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(gal, row, prepared):
    _, view, a, out, batch, galois, count, status, text, launches = row
    st, got, goes_on = gal.check(view, prepared, a, out, batch, galois, count)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == ((PREP if prepared else COEFF) + text if text else ""), got


@pytest.mark.parametrize("view", [GENERAL, OMEGA], ids=["general", "omega-only"])
def test_prepared_call_needs_the_fused_kernels_and_the_coefficient_call_does_not(gal, view):
    assert gal.check(view, False, A, C, BATCH, G3) == (OK, "", True)
    assert gal.check(view, True, A, C, BATCH, G3) == (EUNSUPPORTED, PREP + T_FUSED, False)
    # ... looked at behind the plan and before everything else
    assert gal.check(view, True, None, C, BATCH, [4], 0) == (EUNSUPPORTED, PREP + T_FUSED, False)
    assert gal.check(NULL, True, A, C, BATCH, G3)[:2] == (EINVAL, PREP + ": plan is NULL")


def test_overlap_is_the_intersection_of_the_byte_ranges(gal):
    """out's batch * count rows against the input's batch rows, brute force over row and half-row offsets."""
    seen = set()
    for prepared in (False, True):
        for batch in (1, 2, 3):
            for galois in ([3], [3, 5], [1, 3, 5, 7]):
                count = len(galois)
                for off in range(-(batch * count + 2) * ROW, (batch + 2) * ROW + 1, ROW // 2):
                    out = A + off
                    want = out < A + batch * ROW and A < out + batch * count * ROW
                    st, text, goes_on = gal.check(FUSED, prepared, A, out, batch, galois)
                    assert (st, goes_on) == ((EINVAL, False) if want else (OK, True)), (prepared, batch, count, off)
                    assert text == ((PREP if prepared else COEFF) + T_OVERLAP if want else "")
                    seen.add(want)
    assert seen == {True, False}


# ---- the host helper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 256, 4096, 8192])
def test_galois_element(n):
    m = 2 * n
    assert numtheory.galois_element(n) == 1
    assert numtheory.galois_element(n, conjugate=True) == m - 1
    for step in (1, 2, 7, n // 2 - 1, n // 2, 3 * n):
        g, gi = numtheory.galois_element(n, step), numtheory.galois_element(n, -step)
        assert g == pow(5, step, m) and g * gi % m == 1
        assert g % 2 == 1 and gi % 2 == 1 and 1 <= g < m and 1 <= gi < m
        c = numtheory.galois_element(n, step, conjugate=True)
        assert c == g * (m - 1) % m and c % 2 == 1
