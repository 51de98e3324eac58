"""CPU stepping of the pack / trace step kernel (tests/emu_pack/emu_pack.cpp: polydot_pack_kernel stepped thread by thread with the
kernel's own headers: d = ev - X^rot od formed on the load, sigma_g of d[1] through the transpose image, one forward transform per
term, two inverses, s = ev + X^rot od added at both stores, sigma_g of d[0] through the image and added in) against the stepped
explicit route (the monomial product's stepping, s and d in numpy, the automorphism key switch's stepping on d, the addition of
s), against a numpy statement of X^rot, +-, sigma_g with a trivial key, against the phase of a noise-free key with the oracle's
products, and the entry point's argument list (csrc/api_checks.h: check_pack_step), the hazard tags, the LDS banks of the two
permutations and the sanitizer program, without a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import emu_library
from conftest import P64, ROOT, _make, p64
from test_cmux_emu import TRIVIAL, EmuCmux, monomial_np
from test_extprod_emu import input_rows
from test_gadget2_emu import pair_rows
from test_gadget_emu import MODES, POLICIES, gadget_pairs
from test_galois_emu import sigma
from test_galoisks_emu import EmuGaloisKs, key_rows, noise_free_key, trivial_key
from test_lds_banks import conflict_degree
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FN = "tn_poly_pack_step_prepared_dev"
BATCH = 7
P32 = ctypes.POINTER(ctypes.c_uint32)


def elements(n):
    """The Galois elements of the pack tests: the first two levels' (3, 5), the last level's (n + 1: every odd word negated), the
    conjugation 2n - 1 and one seeded."""
    seeded = int(np.random.default_rng(n).integers(0, 2 * n)) | 1
    return [3, 5, n + 1, 2 * n - 1, seeded]


def rotations(n):
    """No rotation, one place, the first level's n / 2, the last place before the wrap, the negation, the last exponent below 2n
    and one seeded."""
    seeded = int(np.random.default_rng(n + 1).integers(0, 2 * n))
    return [0, 1, n // 2, n - 1, n, 2 * n - 1, seeded]


class EmuPack:
    """The entry points of tests/emu_pack/emu_pack.cpp in tests/emu_pack/_build/libemu_pack.so (brought up to date first: nothing to
    do when the library is newer than its sources and headers); the shapes' threads from tests/emu's library."""

    def __init__(self):
        _make("tests/emu_pack")
        L = self.lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_pack", "_build", "libemu_pack.so"))
        self.emu = emu_library.load()
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_pack_step_prepared.argtypes = [u32, u64, u64, ci, P64, P64, u32, u32, P64, sz, P64, sz, sz, u32, u32]
        L.emu_lwe_embed.argtypes = [u32, u64, P64, P64, sz, u32]
        L.emu_pack_maps.argtypes = [u32, u32, u32, u32, P32, P32]
        L.emu_pack_maps.restype = None
        L.emu_pack_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, u32, u32, vp, vp, sz, sz, sz, u32, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]
        L.emu_lwe_embed_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, sz, u32, ctypes.POINTER(ci), ctypes.c_char_p, sz]
        self.emu.emu_galois_lpt.argtypes = [u32]; self.emu.emu_galois_lpt.restype = u32

    def status(self, n, q, psi, ev, od, rot, g, bhat, terms, w, balanced=False, canonical=False):
        """-> (the stepping's return code, c): 0 ok, 9 a hazard tag.  od None: the trace step."""
        ev = np.ascontiguousarray(ev, dtype=np.uint64)
        batch = ev.shape[0]
        assert ev.shape[1:] == (2, n)
        if od is not None:
            od = np.ascontiguousarray(od, dtype=np.uint64)
            assert od.shape == ev.shape
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (2 * terms, batch * 2 * terms)
        sets = 1 if bhat.shape[0] == 2 * terms else batch
        c = np.empty((batch, 2, n), dtype=np.uint64)
        rc = self.lib.emu_poly_pack_step_prepared(n, q, psi, int(canonical), p64(ev), p64(od) if od is not None else None, rot, g, p64(bhat), sets, p64(c),
                                                  batch, terms, w, int(balanced))
        return rc, c

    def step(self, n, q, psi, ev, od, rot, g, bhat, terms, w, balanced=False, canonical=False):
        """ev, od: (batch, 2, n); bhat: (2 * terms, n) for one shared key or (batch * 2 * terms, n) -> (batch, 2, n)."""
        rc, c = self.status(n, q, psi, ev, od, rot, g, bhat, terms, w, balanced, canonical)
        assert rc == 0, rc
        return c

    def embed(self, n, q, lwe, index):
        lwe = np.ascontiguousarray(lwe, dtype=np.uint64)
        a = np.empty((lwe.shape[0], 2, n), dtype=np.uint64)
        rc = self.lib.emu_lwe_embed(n, q, p64(lwe), p64(a), lwe.shape[0], index)
        assert rc == 0, rc
        return a

    def maps(self, logn, g, rot):
        """-> (image word of every source word under sigma_g, negated), (word of od that X^rot brings to every word, negated)."""
        dst = np.empty(1 << logn, dtype=np.uint32); src = np.empty(1 << logn, dtype=np.uint32)
        self.lib.emu_pack_maps(logn, g, rot, self.threads(logn), dst.ctypes.data_as(P32), src.ctypes.data_as(P32))
        low = np.uint32(0x7fffffff)
        return ((dst & low).astype(np.int64), (dst >> np.uint32(31)).astype(bool)), ((src & low).astype(np.int64), (src >> np.uint32(31)).astype(bool))

    def threads(self, logn):
        return (1 << logn) >> self.emu.emu_galois_lpt(logn)

    def check(self, view, ev, od, rot, g, b, c, sets=1, batch=1, terms=1, base_log=1, flags=0):
        """check_pack_step on the plan view (n, elem_bytes, has_fused, omega_only, q) -> (status, text, goes on to a launch)."""
        return emu_library.api_check(self.lib.emu_pack_api_check, *view, ev, od, rot, g, b, c, sets, batch, terms, base_log, flags)

    def check_embed(self, view, lwe, a, batch=1, index=0):
        return emu_library.api_check(self.lib.emu_lwe_embed_api_check, *view, lwe, a, batch, index)


@pytest.fixture(scope="module")
def pack():
    return EmuPack()


@pytest.fixture(scope="module")
def ks():
    return EmuGaloisKs()


@pytest.fixture(scope="module")
def cmux():
    return EmuCmux()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def sum_and_difference(ev, t, q):
    """s = ev + t, d = ev - t mod q for any words ev and canonical t (q < 2^62: the sums fit 64 bits)."""
    e = np.asarray(ev, dtype=np.uint64) % np.uint64(q)
    return (e + t) % np.uint64(q), (e + (np.uint64(q) - t)) % np.uint64(q)


def stepped_route(ks, cmux, n, q, psi, ev, od, rot, g, bh, terms, w, balanced, canonical):
    """The contract, stepped: the monomial product's stepping on od, s and d in numpy, the automorphism key switch's stepping on d,
    s added in numpy.  od None: the trace step, s = d = ev mod q."""
    t = np.zeros_like(ev) if od is None else cmux.monomial(n, q, od, np.full(ev.shape[0], rot, dtype=np.uint32))
    s, d = sum_and_difference(ev, t, q)
    return (ks.keyswitch(n, q, psi, d, g, bh, terms, w, balanced, canonical) + s) % np.uint64(q)


def case_rows(a, b, first=0):
    """ev from a case's a rows, od from its b rows: (7, 2, n) each, the all-(q - 1) row and unreduced full-width rows in both."""
    return np.ascontiguousarray(a[input_rows(BATCH, 2, first)]), np.ascontiguousarray(b[input_rows(BATCH, 2, first + 1)])


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_stepping_matches_the_stepped_explicit_route(pack, ks, cmux, prep, case, canonical):
    """Batch 7, every (terms, w) of gadget_pairs, a shared key and a key per row, both digit modes, and the trace step for every
    element in every group.  The first (terms, w) pair runs the whole element x rotation product (35 launches) for both key kinds
    and both digit modes; the three later pairs run every element with the rotations in turn (5 launches per group, every
    rotation with every element over the groups).  The whole product for every pair is 560 stepped launches and as many stepped
    routes per case instead of 200, 2.8 times the time of the slowest test of this file, for code paths (the digit count and
    width) that the rotation and the element do not reach."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    gs, rots = elements(n), rotations(n)
    turn = 0
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        ev, od = case_rows(a, b, first)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            for balanced in MODES:
                grid = [(g, r) for g in gs for r in rots] if first == 0 else [(g, rots[(i + turn) % len(rots)]) for i, g in enumerate(gs)]
                turn += 1
                for g, rot in grid:
                    where = (case, canonical, terms, w, shared, balanced, g, rot)
                    c = pack.step(n, q, psi, ev, od, rot, g, bh, terms, w, balanced, canonical)
                    assert np.array_equal(c, stepped_route(ks, cmux, n, q, psi, ev, od, rot, g, bh, terms, w, balanced, canonical)), where
                for g in gs:
                    c = pack.step(n, q, psi, ev, None, 0, g, bh, terms, w, balanced, canonical)
                    assert np.array_equal(c, stepped_route(ks, cmux, n, q, psi, ev, None, 0, g, bh, terms, w, balanced, canonical)), (case, g, "trace")


def trivial_want(ev, od, rot, g, q, component):
    """What a trivial key makes of (ev, od) by the numpy statements of X^rot (tests/test_cmux_emu.py) and sigma_g
    (tests/test_galois_emu.py): nothing here passes through the project's own code."""
    t = np.zeros_like(ev) if od is None else monomial_np(od, np.full(ev.shape[0], rot), q)
    s, d = sum_and_difference(ev, t, q)
    sd = sigma(d, g, q)
    want = s.copy()
    want[:, 0] = (want[:, 0] + sd[:, 0]) % np.uint64(q)
    want[:, component] = (want[:, component] + sd[:, 1]) % np.uint64(q)
    return want


@pytest.mark.parametrize("case", ["P256", "P1024", "P4096_60"])
@POLICIES
def test_trivial_key_returns_the_sum_and_sigma_of_the_difference(pack, prep, case, canonical):
    """Unsigned digits that cover q recompose exactly.  K[1][j] = 2^(j w), K[0] = 0: the output is (s0 + sigma_g(d0), s1 + sigma_g(d1)).
    K[0][j] = 2^(j w), K[1] = 0: it is (s0 + sigma_g(d0) + sigma_g(d1), s1)."""
    n, q, psi, a, b = _case_data(case)
    terms, w = TRIVIAL[q.bit_length()]
    assert terms * w >= q.bit_length() and (1 << w) < q and (terms - 1) * w < 64
    ev, od = case_rows(a, b)
    rots = rotations(n)
    for component in (0, 1):
        bh = prep.prepare(n, q, psi, trivial_key(n, q, component, terms, w), canonical)
        for i, g in enumerate(elements(n)):
            for rot in (rots[i], rots[(i + 3) % len(rots)]):
                c = pack.step(n, q, psi, ev, od, rot, g, bh, terms, w, False, canonical)
                assert np.array_equal(c, trivial_want(ev, od, rot, g, q, component)), (case, canonical, component, g, rot)
            c = pack.step(n, q, psi, ev, None, 0, g, bh, terms, w, False, canonical)
            assert np.array_equal(c, trivial_want(ev, None, 0, g, q, component)), (case, canonical, component, g, "trace")


@pytest.mark.parametrize("case", ["P256", "P1024"])
def test_phase_is_the_sum_plus_sigma_of_the_difference(pack, prep, oracle, case):
    """out0 + out1 s = (ev + t)(s) + sigma_g((ev - t)(s)), exactly, t = X^rot od, for a noise-free key from sigma_g(s) to s and
    unsigned digits that cover q; the products are the oracle's, X^rot and sigma_g the numpy statements."""
    n, q, psi, a, b = _case_data(case)
    terms, w = TRIVIAL[q.bit_length()]
    rng = np.random.default_rng(n + 23)
    s = rng.integers(0, q, n, dtype=np.uint64)
    ev, od = case_rows(a, b)
    srows = np.broadcast_to(s, (BATCH, n)).copy()
    q64 = np.uint64(q)

    def phase(ct):
        return (ct[:, 0] % q64 + oracle.poly_mult(np.ascontiguousarray(ct[:, 1]), srows, q, psi)) % q64

    rots = rotations(n)
    for i, g in enumerate(elements(n)):
        bh = prep.prepare(n, q, psi, noise_free_key(oracle, n, q, psi, s, g, terms, w, g), False)
        for rot, o in ((rots[i], od), (rots[(i + 4) % len(rots)], od), (0, None)):
            t = np.zeros_like(ev) if o is None else monomial_np(o, np.full(BATCH, rot), q)
            ps, pd = sum_and_difference(phase(ev), phase(t), q)
            c = pack.step(n, q, psi, ev, o, rot, g, bh, terms, w, False, False)
            assert np.array_equal(phase(c), (ps + sigma(pd, g, q)) % q64), (case, g, rot, o is None)


@pytest.mark.parametrize("case", ["P256", (256, 1152921504606830593), "P1024", "P4096_60"])
@POLICIES
def test_hazard_tags_report_none(pack, prep, case, canonical):
    """(The tags follow the ORDER of the kernel's steps; the stepping is sequential, so they cannot show that a barrier is present:
    the kernel's READBACK_BARRIER could be removed without this test failing.  tests/test_gpu_pack.py covers it on the device.)
    A workgroup of one wave (n = 256, 32-bit), of more (the others), the base-case shape: the stepping's tags of the three
    hazards on the image (a scatter behind a finished transform, a read-back behind its whole scatter, a transform behind the whole
    read-back) stay silent over several rows, so that one row's second permutation is followed by the next row's first; the
    pack form and the trace form."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    ev, od = a[input_rows(3, 2)], b[input_rows(3, 2, 1)]
    for g, rot in ((3, n // 2), (n + 1, 1), (2 * n - 1, 2 * n - 1)):
        for o, r in ((od, rot), (None, 0)):
            rc, _ = pack.status(n, q, psi, ev, o, r, g, bhat[pair_rows(3, 2).ravel()], 2, q.bit_length() // 2, True, canonical)
            assert rc == 0, (case, canonical, g, r, rc)


def test_stepping_refuses_what_the_entry_point_refuses(pack, prep):
    n, q, psi, a, b = _case_data("P256")
    bh = prep.prepare(n, q, psi, b[:4])
    ev, od = a[input_rows(1, 2)], b[input_rows(1, 2)]
    for rot, g, o in ((2 * n, 3, od), (0, 4, od), (0, 2 * n + 1, od), (1, 3, None)):
        assert pack.status(n, q, psi, ev, o, rot, g, bh, 2, 11)[0] == 5, (rot, g)


def permutation_degrees(pack, logn, word, g):
    """Worst conflict degree of the scatter (a ds write of `word` bytes, lanes g words apart) and of the read-back (a ds read at
    unit stride) over every wave and register of a workgroup of the shape's threads (the bank model of tests/test_lds_banks.py)."""
    n, threads = 1 << logn, pack.threads(logn)
    (dst, _), _ = pack.maps(logn, g, 0)
    worst_w = worst_r = 1
    for r in range(n // threads):
        for wave in range(0, threads, 64):
            lanes = np.arange(wave, min(wave + 64, threads))
            src = r * threads + lanes
            worst_w = max(worst_w, conflict_degree([int(v) * word for v in dst[src]], "write", word))
            worst_r = max(worst_r, conflict_degree([int(v) * word for v in src], "read", word))
    return worst_w, worst_r


@pytest.mark.parametrize("word", [4, 8])
def test_permutations_are_bank_conflict_free_for_every_element_at_n_256(pack, word):
    for g in range(1, 512, 2):
        assert permutation_degrees(pack, 8, word, g) == (1, 1), (word, g)


def test_maps_are_the_definitions(pack):
    """galois_dst against the numpy statement (source word i goes to i g mod 2n, negated from n on) and the rotated load's index
    and sign against X^rot (word i comes from word (i - rot) mod 2n, negated from n on), at the smallest and the largest shape."""
    for logn in (8, 13):
        n = 1 << logn
        i = np.arange(n)
        for g in elements(n):
            for rot in rotations(n):
                (dst, neg), (src, sneg) = pack.maps(logn, g, rot)
                t = i * g % (2 * n)
                assert np.array_equal(dst, t % n) and np.array_equal(neg, t >= n), (n, g)
                assert len(set(dst.tolist())) == n
                v = (i - rot) % (2 * n)
                assert np.array_equal(src, v % n) and np.array_equal(sneg, v >= n), (n, rot)


# ---- the argument list -------------------------------------------------------------------------
N, WORD, Q, W = 4, 4, 7681, 4                               # the smallest plan: rows of 16 bytes; 2^W < Q
ROW = N * WORD
FUSED, GENERAL, NULL = (N, WORD, 1, 0, Q), (N, WORD, 0, 0, Q), (0, 0, 0, 0, 0)
A, D, B, C = 1 << 20, 1 << 25, 1 << 30, 1 << 40
BATCH_, TERMS, G, ROT = 5, 2, 3, 2
T_ROWS = FN + ": batch * 2 * terms too large for one call (max 2^31 - 1 digit rows)"
T_OVERLAP = FN + ": output must not alias or overlap an input"
T_FUSED = FN + ": prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_SETS = FN + ": bhat_sets must be 1 (one set of operands for every row) or batch"
T_BASE = FN + ": need 1 <= base_log and 2^base_log < q"
T_EVEN = FN + ": galois[0] = 4 is not an odd element below 2n"
T_ROT = FN + ": rot = 8 is not below 2n"
T_TRACE = FN + ": rot must be 0 when od is NULL (the trace step)"
SET = 2 * TERMS                                             # rows of one key

# (id, view, ev, od, bhat, c, keywords, status, text or None, goes on to a launch)
TABLE = [
    ("ok", FUSED, A, D, B, C, {}, OK, None, True),
    ("shared-ok", FUSED, A, D, B, C, dict(sets=1), OK, None, True),
    ("balanced-ok", FUSED, A, D, B, C, dict(flags=1), OK, None, True),
    ("rot-0-ok", FUSED, A, D, B, C, dict(rot=0), OK, None, True),
    ("rot-2n-minus-1-ok", FUSED, A, D, B, C, dict(rot=2 * N - 1), OK, None, True),
    ("trace-ok", FUSED, A, None, B, C, dict(rot=0), OK, None, True),
    ("ev-is-od-ok", FUSED, A, A, B, C, {}, OK, None, True),
    # one row per fault, in the order of the list
    ("null-plan", NULL, A, D, B, C, {}, EINVAL, FN + ": plan is NULL", False),
    ("general-plan", GENERAL, A, D, B, C, {}, EUNSUPPORTED, T_FUSED, False),
    ("galois-even", FUSED, A, D, B, C, dict(g=4), EINVAL, T_EVEN, False),
    ("galois-2n-plus-1", FUSED, A, D, B, C, dict(g=2 * N + 1), EINVAL, FN + ": galois[0] = 9 is not an odd element below 2n", False),
    ("rot-2n", FUSED, A, D, B, C, dict(rot=2 * N), EINVAL, T_ROT, False),
    ("trace-with-a-rotation", FUSED, A, None, B, C, dict(rot=1), EINVAL, T_TRACE, False),
    ("terms-0", FUSED, A, D, B, C, dict(terms=0), EINVAL, FN + ": terms must be at least 1", False),
    ("flag-2", FUSED, A, D, B, C, dict(flags=2), EINVAL, FN + ": unknown flag bit", False),
    ("base-log-0", FUSED, A, D, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("base-log-k", FUSED, A, D, B, C, dict(base_log=13), EINVAL, T_BASE, False),
    ("shift-64", FUSED, A, D, B, C, dict(terms=65, base_log=1), EINVAL, FN + ": (terms - 1) * base_log must be below 64", False),
    ("rows-2^31", FUSED, 4096, 4096, 4096, 4096, dict(sets=1, batch=2 ** 29, terms=2, base_log=1), EINVAL, T_ROWS, False),
    ("rows-2^31-minus-2", FUSED, A, 1 << 45, 1 << 50, 1 << 58, dict(sets=1, batch=2 ** 30 - 1, terms=1), OK, None, True),
    ("batch0-null", FUSED, None, None, None, None, dict(batch=0, sets=1, rot=0), OK, None, False),
    ("null-ev", FUSED, None, D, B, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-bhat", FUSED, A, D, None, C, {}, EINVAL, FN + ": NULL buffer", False),
    ("null-c", FUSED, A, D, B, None, {}, EINVAL, FN + ": NULL buffer", False),
    ("sets-2", FUSED, A, D, B, C, dict(sets=2), EINVAL, T_SETS, False),
    # overlap by byte range: c's batch * 2 rows against ev's and od's batch * 2 rows ...
    ("c-is-ev", FUSED, A, D, B, A, {}, EINVAL, T_OVERLAP, False),
    ("c-is-od", FUSED, A, D, B, D, {}, EINVAL, T_OVERLAP, False),
    ("c-over-last-row-of-od", FUSED, A, D, B, D + (BATCH_ * 2 - 1) * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-last-byte-is-first-of-od", FUSED, A, D, B, D - BATCH_ * 2 * ROW + 1, {}, EINVAL, T_OVERLAP, False),
    ("c-just-before-od", FUSED, A, D, B, D - BATCH_ * 2 * ROW, {}, OK, None, True),
    ("c-just-past-od", FUSED, A, D, B, D + BATCH_ * 2 * ROW, {}, OK, None, True),
    ("c-just-past-ev", FUSED, A, D, B, A + BATCH_ * 2 * ROW, {}, OK, None, True),
    ("c-where-od-would-be-in-a-trace-step", FUSED, A, None, B, D, dict(rot=0), OK, None, True),
    # ... against a shared key's 2 * terms rows and the batch keys of a launch with a key per row
    ("c-over-last-row-of-the-key", FUSED, A, D, B, B + (SET - 1) * ROW, dict(sets=1), EINVAL, T_OVERLAP, False),
    ("c-just-past-the-key", FUSED, A, D, B, B + SET * ROW, dict(sets=1), OK, None, True),
    ("c-past-the-first-key-of-the-keys", FUSED, A, D, B, B + SET * ROW, {}, EINVAL, T_OVERLAP, False),
    ("c-just-past-the-keys", FUSED, A, D, B, B + BATCH_ * SET * ROW, {}, OK, None, True),
    # two faults: the order (plan, kernels, galois, rot, terms, flags, base_log, shift, rows, batch 0, buffers, sets, overlap)
    ("null-plan-galois-even", NULL, A, D, B, C, dict(g=4), EINVAL, FN + ": plan is NULL", False),
    ("general-plan-rot-2n", GENERAL, A, D, B, C, dict(rot=2 * N), EUNSUPPORTED, T_FUSED, False),
    ("galois-even-rot-2n", FUSED, A, D, B, C, dict(g=4, rot=2 * N), EINVAL, T_EVEN, False),
    ("rot-2n-terms-0", FUSED, A, D, B, C, dict(rot=2 * N, terms=0), EINVAL, T_ROT, False),
    ("rot-2n-in-a-trace-step", FUSED, A, None, B, C, dict(rot=2 * N), EINVAL, T_ROT, False),
    ("trace-rotation-batch-0", FUSED, None, None, None, None, dict(rot=1, batch=0, sets=1), EINVAL, T_TRACE, False),
    ("terms-0-flag-2", FUSED, A, D, B, C, dict(terms=0, flags=2), EINVAL, FN + ": terms must be at least 1", False),
    ("base-log-0-null-ev", FUSED, None, D, B, C, dict(base_log=0), EINVAL, T_BASE, False),
    ("rows-null-ev", FUSED, None, 4096, 4096, 4096, dict(sets=1, batch=2 ** 31), EINVAL, T_ROWS, False),
    ("batch0-sets-2", FUSED, A, D, B, C, dict(batch=0, sets=2), OK, None, False),
    ("null-ev-sets-2", FUSED, None, D, B, C, dict(sets=2), EINVAL, FN + ": NULL buffer", False),
    ("sets-2-c-is-ev", FUSED, A, D, B, A, dict(sets=2), EINVAL, T_SETS, False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(pack, row):
    _, view, ev, od, b, c, kw, status, text, launches = row
    full = dict(g=G, rot=ROT, sets=BATCH_, batch=BATCH_, terms=TERMS, base_log=W, flags=0)
    full.update(kw)
    g, rot = full.pop("g"), full.pop("rot")
    st, got, goes_on = pack.check(view, ev, od, rot, g, b, c, **full)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got


def test_overlap_is_the_intersection_of_the_byte_ranges(pack):
    """c's batch * 2 rows against ev's and od's batch * 2 rows and against the key's sets * 2 * terms rows, every half row around them."""
    for batch in (1, 2):
        for terms in (1, 2):
            for sets in (1, batch):
                for which, in_rows in (("ev", batch * 2), ("od", batch * 2), ("bhat", sets * 2 * terms)):
                    for off in range(-5 * ROW, (in_rows + 2) * ROW + 1, ROW // 2):
                        out = A + off
                        want = out < A + in_rows * ROW and A < out + batch * 2 * ROW
                        ev, od, b = {"ev": (A, D, B), "od": (D, A, B), "bhat": (B, D, A)}[which]
                        st, text, goes_on = pack.check(FUSED, ev, od, ROT, G, b, out, sets=sets, batch=batch, terms=terms, base_log=W)
                        assert (st, goes_on) == ((EINVAL, False) if want else (OK, True)), (batch, terms, sets, which, off)
                        assert text == (T_OVERLAP if want else "")


def test_sanitizer_program_runs_clean():
    """The stepping's cases (tests/emu_pack/emu_pack.cpp, behind EMU_SANITIZE_CASES) under AddressSanitizer + UBSan: n = 256 at both lane
    widths and n = 4096 / 60-bit, both policies, batch 2 x 2 terms, a shared key and a key per row, both digit modes, six (g, rot)
    pairs and the trace step, each against the stepped monomial product, 128-bit host sums, the stepped key switch and the
    addition (4 checks each, 3 for the trace step: 648); the embedding on exactly sized buffers (18); the argument list on made-up
    addresses (362).  A stand-alone program of its own (tests/emu_pack/sanitize_pack.cpp): nothing is loaded into Python."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_pack")
    b = subprocess.run(["make", "-j8", "-C", d, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-2000:]
    r = subprocess.run([os.path.join(d, "_build", "sanitize_pack")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    counts = {name: int(v) for name, v in re.findall(r"^(\w+): (\d+) checks$", r.stdout, re.M)}
    assert counts == {"pack": 1028}, counts
    assert re.search(r"^sanitize_pack: 1028 checks, 0 failures$", r.stdout, re.M), r.stdout[-500:]
