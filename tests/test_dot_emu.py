"""CPU stepping of the prepared dot-product kernel (tests/emu/emu_dot.cpp: polydot_prepared_kernel stepped thread by thread
with the kernel's own headers, accumulate function and prepared-order index map) against the oracle, without a GPU."""
import ctypes

import numpy as np
import pytest

import emu_library
from conftest import PARAMS, P64, ntt_prime_below, p64
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data, operand_rows

POLICIES = pytest.mark.parametrize("canonical", [False, True], ids=["lazy", "canonical"])


class EmuDot:
    """The prepared dot-product entry points of tests/emu/_build/libemu.so (tests/emu/emu_dot.cpp)."""

    def __init__(self):
        L = self.lib = emu_library.load()
        u32, u64, sz, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        L.emu_poly_dot_prepared.argtypes = [u32, u64, u64, ci, P64, P64, sz, P64, sz, sz]
        L.emu_dot_accumulate.argtypes = [u32, u64, u64, ci, P64, P64, P64, sz, ctypes.POINTER(ci), ctypes.POINTER(ci)]

    def poly_dot_prepared(self, n, q, psi, a, bhat, canonical=False):
        """a: (batch, terms, n); bhat: (terms, n) for one shared set or (batch * terms, n)."""
        a = np.ascontiguousarray(a, dtype=np.uint64)
        batch, terms = a.shape[0], a.shape[1]
        bhat = np.ascontiguousarray(bhat, dtype=np.uint64).reshape(-1, n)
        assert bhat.shape[0] in (terms, batch * terms)
        sets = 1 if bhat.shape[0] == terms else batch
        c = np.empty((batch, n), dtype=np.uint64)
        rc = self.lib.emu_poly_dot_prepared(n, q, psi, int(canonical), p64(a), p64(bhat), sets, p64(c), batch, terms)
        assert rc == 0, rc
        return c

    def accumulate(self, n, q, psi, acc, x, canonical=False):
        """Element-wise dot_accumulate_one of the plan's lane width and policy -> (out, lane bytes, lazy)."""
        acc = np.ascontiguousarray(acc, dtype=np.uint64)
        x = np.ascontiguousarray(x, dtype=np.uint64)
        out = np.empty_like(acc)
        lane, lazy = ctypes.c_int(), ctypes.c_int()
        rc = self.lib.emu_dot_accumulate(n, q, psi, int(canonical), p64(acc), p64(x), p64(out), acc.size, ctypes.byref(lane), ctypes.byref(lazy))
        assert rc == 0, rc
        return out, lane.value, bool(lazy.value)


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def term_rows(batch, terms, rows=5):
    """Index of the case's row that term j of output row r takes: the case's rows, cyclically."""
    return (np.arange(batch * terms) % rows).reshape(batch, terms)


def sum_mod(products, q):
    """Sum over axis 1 of canonical residues, mod q (terms * q < 2^64 for every modulus and term count used here)."""
    assert products.shape[1] * q < 2 ** 64
    return products.sum(axis=1, dtype=np.uint64) % np.uint64(q)


@pytest.fixture(scope="module")
def products(oracle):
    """The oracle's products a[i] * b[k] of a case's rows, i < 5, k < 5 on the diagonal and k < 3 elsewhere: what the terms of
    the parity tests are taken from.  Computed once per case and left unchanged."""
    cache = {}

    def get(case):
        if case not in cache:
            n, q, psi, a, b = _case_data(case)
            pairs = sorted({(i, i) for i in range(5)} | {(i, k) for i in range(5) for k in range(3)})
            ia, ib = [i for i, _ in pairs], [k for _, k in pairs]
            ref = oracle.poly_mult(a[ia], b[ib], q, psi)
            ref.setflags(write=False)
            cache[case] = {pair: ref[t] for t, pair in enumerate(pairs)}
        return cache[case]
    return get


def dot_reference(prods, q, idx, shared):
    """Sum of the oracle's products for the term layout idx; shared: term j is multiplied by b[j], otherwise by b[idx]."""
    batch, terms = idx.shape
    rows = [[prods[(int(idx[r, j]), j if shared else int(idx[r, j]))] for j in range(terms)] for r in range(batch)]
    return sum_mod(np.array(rows, dtype=np.uint64), q)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_dot_product_matches_the_sum_of_oracle_products(dot, prep, products, case, canonical):
    """terms 1, 2, 3 at batch 2, the terms taken cyclically from the case's rows (full-width unreduced words, the all-(q - 1) row
    and x^(n-1) * x = -1 among them); one shared set of prepared rows, and one set per output row."""
    n, q, psi, a, b = _case_data(case)
    prods = products(case)
    assert prods[(4, 4)][0] == q - 1 and not prods[(4, 4)][1:].any()          # x^(n-1) * x = -1
    bhat = prep.prepare(n, q, psi, b, canonical)
    for terms in (1, 2, 3):
        idx = term_rows(2, terms)
        c = dot.poly_dot_prepared(n, q, psi, a[idx], bhat[idx].reshape(-1, n), canonical)
        assert np.array_equal(c, dot_reference(prods, q, idx, False)), (case, canonical, terms, "per set")
        c = dot.poly_dot_prepared(n, q, psi, a[idx], bhat[:terms], canonical)
        assert np.array_equal(c, dot_reference(prods, q, idx, True)), (case, canonical, terms, "shared")
    bad = dot.lib.emu_poly_dot_prepared(n, q, psi, int(canonical), p64(np.ascontiguousarray(a[term_rows(3, 2)])), p64(np.ascontiguousarray(bhat[:4])), 2,
                                        p64(np.empty((3, n), dtype=np.uint64)), 3, 2)
    assert bad == 3                                                            # bhat_sets is neither 1 nor batch


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@POLICIES
def test_opposite_terms_cancel(dot, prep, case, canonical):
    """terms = 2, a[r][1] = -a[r][0] mod q, the same b for both terms: every word of c is 0."""
    n, q, psi, a, b = _case_data(case)
    a0 = a[:2]
    a1 = (np.uint64(q) - a0 % np.uint64(q)) % np.uint64(q)
    pair = np.stack([a0, a1], axis=1)                                          # (2, 2, n)
    bhat = prep.prepare(n, q, psi, b[:1], canonical)
    c = dot.poly_dot_prepared(n, q, psi, pair, np.repeat(bhat, 2, axis=0), canonical)
    assert not c.any(), (case, canonical)
    per_set = prep.prepare(n, q, psi, b[[0, 0, 1, 1]], canonical)
    c = dot.poly_dot_prepared(n, q, psi, pair, per_set, canonical)
    assert not c.any(), (case, canonical)


@pytest.mark.parametrize("case", ["P4096_60", "P1024"])
@POLICIES
def test_sum_wraps_on_every_term(dot, prep, oracle, case, canonical):
    """terms = 7, every word of a and b equal to q - 1: the running sum wraps mod q on every term."""
    n, q, psi, _, _ = _case_data(case)
    terms = 7
    ones = np.full((1, n), q - 1, dtype=np.uint64)
    one = oracle.poly_mult(ones, ones, q, psi)
    assert int(one[0, 0]) == q - (n - 2)           # (1 + x + ... + x^(n-1))^2 has 2k + 2 - n at x^k: the low words are just below q,
    ref = sum_mod(np.repeat(one[:, None, :], terms, axis=1), q)     # so from the second term on every addition to them wraps
    a = np.full((2, terms, n), q - 1, dtype=np.uint64)
    bhat = prep.prepare(n, q, psi, np.repeat(ones, terms, axis=0), canonical)
    c = dot.poly_dot_prepared(n, q, psi, a, bhat, canonical)
    assert np.array_equal(c, np.repeat(ref, 2, axis=0)), (case, canonical)
    c = dot.poly_dot_prepared(n, q, psi, a, np.repeat(bhat, 2, axis=0), canonical)
    assert np.array_equal(c, np.repeat(ref, 2, axis=0)), (case, canonical)


@pytest.mark.parametrize("case", ["P4096_60", "P1024"])
@POLICIES
def test_accumulate_contract(dot, case, canonical):
    """dot_accumulate_one: acc in [0, q) and x anywhere in the output range of the plan's product -> a word in [0, q) equal to
    (acc + x) mod q.  The range's edges are 0, q - 1, q, 2q - 1 (64-bit lazy lanes: pointwise() stays below 2q) and 4q - 1
    (32-bit lazy lanes: below 4q); the 64-bit lazy plan with the base case adds that product's bound, 9.75 * 2^k, rounded up
    to 10 * 2^k - 1.  The canonical policy's product is canonical, so its range ends at q - 1: that policy's function adds and
    subtracts once, and a word from q on is outside its precondition."""
    n, q, psi = PARAMS[case]
    _, lane, lazy = dot.accumulate(n, q, psi, [0], [0], canonical)
    assert lazy == (not canonical) and lane == (8 if q > 2 ** 32 else 4)
    if not lazy:
        bound = q
    elif lane == 4:
        bound = 4 * q
    else:
        bound = 10 * 2 ** q.bit_length()
    edges = sorted({e for e in (0, q - 1, q, 2 * q - 1, 4 * q - 1, bound - 1) if e < bound})
    assert len(edges) == (2 if not lazy else 5 if lane == 4 else 6)
    rng = np.random.default_rng(q % 1000 + canonical)
    acc = [s for s in (0, 1, q - 1) for _ in edges] + [int(v) for v in rng.integers(0, q, 2000, dtype=np.uint64)]
    x = [e for _ in (0, 1, q - 1) for e in edges] + [int(v) for v in rng.integers(0, bound, 2000, dtype=np.uint64)]
    out, _, _ = dot.accumulate(n, q, psi, acc, x, canonical)
    for s, v, o in zip(acc, x, out):
        assert int(o) < q and int(o) == (s + v) % q, (case, canonical, s, v, int(o))


def test_generic_modulus_runs_the_canonical_policy(dot, prep, emu, oracle):
    """A 61-bit prime that is not of the form 2^k - c: the plan is not lazy; terms = 3."""
    from tiny_ntt_amd import numtheory
    n = 1024
    q = ntt_prime_below(2 ** 61, n)
    psi = numtheory.primitive_2n_root(n, q)
    assert emu.lib.emu_is_lazy(n, q, psi) == 0
    a, b = operand_rows(n, q, 61)
    idx = term_rows(2, 3)
    bhat = prep.prepare(n, q, psi, b)
    ref = sum_mod(oracle.poly_mult(a[idx.ravel()], b[idx.ravel()], q, psi).reshape(2, 3, n), q)
    assert np.array_equal(dot.poly_dot_prepared(n, q, psi, a[idx], bhat[idx].reshape(-1, n)), ref)
    shared = np.tile(np.arange(3), 2)
    ref = sum_mod(oracle.poly_mult(a[idx.ravel()], b[shared], q, psi).reshape(2, 3, n), q)
    assert np.array_equal(dot.poly_dot_prepared(n, q, psi, a[idx], bhat[:3]), ref)
    _, lane, lazy = dot.accumulate(n, q, psi, [0], [0])
    assert (lane, lazy) == (8, False)


def test_row_plan_of_the_dot_kernel_keeps_32_kib_per_atomic(emu):
    """One output row is `terms` operand rows of work: plan_rows is given terms * n * w bytes per row (launch_plan.h
    dot_row_bytes), and a chunk is the fewest output rows that hold at least 32 KiB of a, never one short row per atomic."""
    L = emu.lib
    sz, ci = ctypes.c_size_t, ctypes.c_int
    L.emu_row_policy.argtypes = [ci, ci]; L.emu_row_policy.restype = ctypes.c_long
    L.emu_plan_rows.argtypes = [ci, sz, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    chunk_bytes, min_chunks = L.emu_row_policy(0, 0), L.emu_row_policy(0, 1)
    assert (chunk_bytes, min_chunks) == (32768, 4)
    for n, w in ((256, 4), (1024, 4), (1024, 8), (2048, 8), (4096, 8), (8192, 8)):
        for terms in (2, 3, 4, 5, 7):
            row_bytes = terms * n * w
            for resident in (1, 512, 1024):
                chunk = ctypes.c_uint32()
                assert L.emu_plan_rows(0, row_bytes, 10 ** 9, resident, ctypes.byref(chunk)) == 1
                assert chunk.value * row_bytes >= chunk_bytes > (chunk.value - 1) * row_bytes, (n, w, terms)
                edge = min_chunks * resident * chunk.value
                assert L.emu_plan_rows(0, row_bytes, edge, resident, ctypes.byref(chunk)) == 1
                assert L.emu_plan_rows(0, row_bytes, edge - 1, resident, ctypes.byref(chunk)) == 0 and chunk.value == 1
