"""CPU stepping of the prepared-operand kernels (tests/emu/emu_prepared.cpp: prepare_fused_kernel and polymul_prepared_kernel
stepped thread by thread with the kernels' own headers and prepared-order index map) against the oracle and against the
stepping of the three-transform product kernel, without a GPU."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import emu_library
from conftest import GOLDEN, PARAMS, P64, ntt_prime_below, p64

Q23, Q60 = 8380417, 1152921504606830593          # the reference's two moduli


class EmuPrepared:
    """The prepared-operand entry points of tests/emu/_build/libemu.so (tests/emu/emu_prepared.cpp)."""

    def __init__(self):
        L = self.lib = emu_library.load()
        u32, u64, sz, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_prepare.argtypes = [u32, u64, u64, ci, P64, P64, sz]
        L.emu_poly_mult_prepared.argtypes = [u32, u64, u64, ci, P64, P64, sz, P64, sz]

    def prepare(self, n, q, psi, b, canonical=False):
        b = np.atleast_2d(np.ascontiguousarray(b, dtype=np.uint64))
        bhat = np.empty_like(b)
        rc = self.lib.emu_prepare(n, q, psi, int(canonical), p64(b), p64(bhat), b.shape[0])
        assert rc == 0, rc
        return bhat

    def poly_mult_prepared(self, n, q, psi, a, bhat, canonical=False):
        a = np.atleast_2d(np.ascontiguousarray(a, dtype=np.uint64))
        bhat = np.atleast_2d(np.ascontiguousarray(bhat, dtype=np.uint64))
        c = np.empty_like(a)
        rc = self.lib.emu_poly_mult_prepared(n, q, psi, int(canonical), p64(a), p64(bhat), bhat.shape[0], p64(c), a.shape[0])
        assert rc == 0, rc
        return c


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def shape_params(case):
    """(n, q, psi) of a case: a tag of conftest.PARAMS, (n, q) with psi found for it, or the n = 8192 golden file's."""
    if case == "P8192_60":
        with open(os.path.join(GOLDEN, "golden_P8192_60.json")) as f:
            meta = json.load(f)
        return meta["n"], meta["q"], meta["psi"]
    if isinstance(case, str):
        return PARAMS[case]
    from tiny_ntt_amd import numtheory
    n, q = case
    return n, q, numtheory.primitive_2n_root(n, q)


CASES = ["P256", "P1024", "P4096", "P4096_60", (512, Q23), (512, Q60), (2048, Q23), (2048, Q60), "P8192_60"]
CASE_IDS = [c if isinstance(c, str) else f"n{c[0]}_q{c[1].bit_length()}" for c in CASES]


def operand_rows(n, q, seed):
    """3 random rows of full-width (unreduced) words, one row of all q - 1, one row a = x^(n-1), b = x (wraps: c[0] = q - 1)."""
    rng = np.random.default_rng(seed)
    word = 2 ** 32 - 1 if q < 2 ** 31 else 2 ** 64 - 1
    a = rng.integers(0, word, (5, n), dtype=np.uint64, endpoint=True)
    b = rng.integers(0, word, (5, n), dtype=np.uint64, endpoint=True)
    a[3] = q - 1; b[3] = q - 1
    a[4] = 0; a[4, n - 1] = 1
    b[4] = 0; b[4, 1] = 1
    return a, b


@functools.lru_cache(maxsize=None)
def _case_data(case):
    n, q, psi = shape_params(case)
    a, b = operand_rows(n, q, n + q % 1000)
    for arr in (a, b):
        arr.setflags(write=False)
    return n, q, psi, a, b


@pytest.fixture(scope="module")
def reference(oracle):
    """The oracle's products of a case's rows, computed once per case and left unchanged."""
    cache = {}

    def get(case):
        if case not in cache:
            n, q, psi, a, b = _case_data(case)
            ref = oracle.poly_mult(a, b, q, psi)
            ref.setflags(write=False)
            cache[case] = ref
        return cache[case]
    return get


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])
def test_prepared_product_matches_oracle_and_fused_stepping(prep, emu, reference, case, canonical):
    n, q, psi, a, b = _case_data(case)
    ref = reference(case)
    assert ref[4, 0] == q - 1 and not ref[4, 1:].any()                    # x^(n-1) * x = -1
    bhat = prep.prepare(n, q, psi, b, canonical)
    c = prep.poly_mult_prepared(n, q, psi, a, bhat, canonical)
    fused = emu.fused(n, q, psi, a, b, canonical=canonical)
    for r in range(a.shape[0]):
        assert np.array_equal(c[r], ref[r]), (case, canonical, r)
        assert np.array_equal(c[r], fused[r]), (case, canonical, r)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])
def test_shared_prepared_operand(prep, oracle, case, canonical):
    """bhat_rows = 1: five different rows of a, each multiplied by b[0]."""
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b[:1], canonical)
    assert bhat.shape == (1, n)
    c = prep.poly_mult_prepared(n, q, psi, a, bhat, canonical)
    ref = oracle.poly_mult(a, np.repeat(b[:1], a.shape[0], axis=0), q, psi)
    for r in range(a.shape[0]):
        assert np.array_equal(c[r], ref[r]), (case, canonical, r)
    assert prep.lib.emu_poly_mult_prepared(n, q, psi, int(canonical), p64(np.ascontiguousarray(a)), p64(np.repeat(bhat, 2, axis=0)), 2, p64(np.empty_like(a)), 5) == 3


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])
def test_prepared_words_are_canonical_and_depend_on_b_mod_q_only(prep, case, canonical):
    n, q, psi, a, b = _case_data(case)
    bhat = prep.prepare(n, q, psi, b, canonical)
    assert int(bhat.max()) < q
    assert np.array_equal(bhat, prep.prepare(n, q, psi, b % np.uint64(q), canonical))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])
def test_prepared_row_is_the_complete_transform_where_no_base_case_runs(prep, emu, case, canonical):
    """Content independent of layout: without the base case a prepared row is a permutation of twist + forward transform.
    Among CASES exactly one plan takes the base case; tests/policy_moduli.py lists more (n = 4096, 50 to 60 bits) and
    tests/test_policy_moduli_emu.py runs them."""
    n, q, psi, a, b = _case_data(case)
    emu.lib.bc_enabled.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
    bc_plan = emu.lib.bc_enabled(n, q, psi) == 1
    assert bc_plan == (case == "P4096_60")              # among CASES the base-case path is taken by exactly this plan
    bhat = prep.prepare(n, q, psi, b, canonical)
    complete = [np.sort(emu.fused_ntt(n, q, psi, 0, b[r], canonical)) for r in range(b.shape[0])]
    if bc_plan and not canonical:                       # (a canonical-policy plan never runs the base case)
        assert any(not np.array_equal(np.sort(bhat[r]), complete[r]) for r in range(3))      # stopped one stage early
        return
    for r in range(b.shape[0]):
        assert np.array_equal(np.sort(bhat[r]), complete[r]), (case, canonical, r)


def test_generic_modulus_runs_the_canonical_policy(prep, emu, oracle):
    """A 61-bit prime that is not of the form 2^k - c: the plan is not lazy, the kernels run the canonical policy."""
    from tiny_ntt_amd import numtheory
    n = 1024
    q = ntt_prime_below(2 ** 61, n)
    psi = numtheory.primitive_2n_root(n, q)
    assert emu.lib.emu_is_lazy(n, q, psi) == 0
    a, b = operand_rows(n, q, 61)
    ref = oracle.poly_mult(a, b, q, psi)
    bhat = prep.prepare(n, q, psi, b)
    assert int(bhat.max()) < q
    assert np.array_equal(prep.poly_mult_prepared(n, q, psi, a, bhat), ref)
    assert np.array_equal(prep.poly_mult_prepared(n, q, psi, a, bhat[:1]), oracle.poly_mult(a, np.repeat(b[:1], 5, axis=0), q, psi))
    assert np.array_equal(bhat, prep.prepare(n, q, psi, b, canonical=True))
