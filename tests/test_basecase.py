"""Base case of the fused product kernel's incomplete transform (fused_core.h basecase(), modarith.h split_rec(), the exact
replay h_bc_sched_ok() in plan_tables.h), stepped on the CPU by the base-case instantiation of the product stepping in
tests/emu/emu_kernels.cpp: golden products, the oracle, unreduced and q - 1 inputs, the base case on arbitrary 64-bit words,
and which moduli the replay accepts."""
import ctypes
import random

import numpy as np
import pytest

from conftest import PARAMS, P64, ntt_prime_below, p64


@pytest.fixture(scope="module")
def bc(emu):
    L = emu.lib
    u32, u64, sz, ci = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    L.bc_enabled.argtypes = [u32, u64, u64]
    L.bc_sched_ok.argtypes = [u32, ci, u64]
    L.split_sched_ok.argtypes = [u32, ci, u64]
    L.bc_polymul.argtypes = [u32, u64, u64, P64, P64, P64, sz, ci]
    L.bc_pair.argtypes = [ci, u64, u64, u64, u64, u64, u64, P64]
    L.bc_split_rec.argtypes = [ci, u64, u64, P64]
    return L


def polymul(bc, n, q, psi, a, b, cyclic=False):
    shape = np.shape(a)
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, n); b = np.ascontiguousarray(b, dtype=np.uint64).reshape(-1, n)
    assert a.shape == b.shape
    c = np.empty_like(a)
    assert bc.bc_polymul(n, q, psi, p64(a), p64(b), p64(c), a.shape[0], int(cyclic)) == 0
    return c.reshape(shape)


def test_reference_modulus_takes_the_base_case(bc):
    assert bc.bc_enabled(*PARAMS["P4096_60"]) == 1
    for tag in ("P256", "P1024", "P4096"):            # other shapes and 32-bit lanes keep the pointwise product
        assert bc.bc_enabled(*PARAMS[tag]) == 0, tag


def test_basecase_matches_golden(bc, golden):
    g = golden("P4096_60")
    for name in g.cases("poly_mult"):
        assert np.array_equal(polymul(bc, g.n, g.q, g.psi, g[name + "_a"], g[name + "_b"]), g[name + "_c"]), name


def test_basecase_random_unreduced_and_extreme_vs_oracle(bc, oracle):
    n, q, psi = PARAMS["P4096_60"]
    rng = np.random.default_rng(11)
    word = 2 ** 64 - 1
    a = rng.integers(0, q, (6, n), dtype=np.uint64); b = rng.integers(0, q, (6, n), dtype=np.uint64)
    a[0] = q - 1; b[0] = q - 1
    a[1] = rng.integers(0, word, n, dtype=np.uint64, endpoint=True); b[1] = word      # any word is taken mod q
    a[2] = word; b[2] = word
    a[3] = q; b[3] = rng.integers(q, word, n, dtype=np.uint64, endpoint=True)
    a[4] = 0
    assert np.array_equal(polymul(bc, n, q, psi, a, b), oracle.poly_mult(a, b, q, psi))


def test_basecase_cyclic_matches_pointwise_path(bc, emu):
    n, q, psi = PARAMS["P4096_60"]
    rng = np.random.default_rng(12)
    a = rng.integers(0, 2 ** 64 - 1, (2, n), dtype=np.uint64, endpoint=True); b = rng.integers(0, q, (2, n), dtype=np.uint64)
    b[1] = q - 1
    assert np.array_equal(polymul(bc, n, q, psi, a, b, cyclic=True), emu.fused(n, q, psi, a, b, cyclic=True))


@pytest.mark.parametrize("k,c", [(60, 2 ** 14 - 1), (60, 1), (52, 2 ** 20 - 3), (47, 2 ** 11 + 1), (57, 12345)])
def test_split_rec_any_word(bc, k, c):
    q = 2 ** k - c
    rng = random.Random(k * 7 + c)
    out = (ctypes.c_uint64 * 2)()
    for b in [0, 1, q - 1, q, 2 * q - 1, 2 ** 64 - 1] + [rng.getrandbits(64) for _ in range(2000)]:
        bc.bc_split_rec(k, c, b, out)
        assert out[0] == b % q                                        # w canonical
        assert out[1] % q == (b << 32) % q and out[1] < 2 ** 32 * c + 2 ** k


def test_basecase_pair_any_word(bc):
    """b0, b1: any 64-bit word; a0, a1: any word below the forward transform's output bound (the schedule folds above it)."""
    k, c = 60, 2 ** 14 - 1
    q = 2 ** k - c
    rng = random.Random(5)
    amax = 7 * 2 ** k                      # SplitSched: forward outputs of the n = 4096 schedule are below 7 * 2^60
    out = (ctypes.c_uint64 * 2)()
    edge_a = [0, 1, q - 1, q, amax - 1]
    edge_b = [0, 1, q - 1, q, 2 ** 64 - 1]
    cases = [(a0, a1, b0, b1) for a0 in edge_a for a1 in edge_a for b0 in edge_b for b1 in edge_b]
    cases += [(rng.randrange(amax), rng.randrange(amax), rng.getrandbits(64), rng.getrandbits(64)) for _ in range(3000)]
    for a0, a1, b0, b1 in cases:
        z = rng.randrange(q)
        bc.bc_pair(k, c, a0, a1, b0, b1, z, out)
        assert out[0] % q == (a0 * b0 + z * a1 * b1) % q and out[1] % q == (a0 * b1 + a1 * b0) % q


def test_replay_accepts_and_rejects(bc):
    # the reference modulus and moduli just below 2^60 with small c pass
    assert bc.bc_sched_ok(12, 60, 2 ** 14 - 1) == 1
    assert bc.bc_sched_ok(12, 60, 1) == 1
    # only n = 4096 has the base-case kernel
    for logn in (8, 10, 11, 13):
        assert bc.bc_sched_ok(logn, 60, 2 ** 14 - 1) == 0
    # outside the split policy's range, or c too large for the records' bounds: rejected (the plan keeps the pointwise kernel)
    assert bc.bc_sched_ok(12, 61, 1) == 0
    assert bc.bc_sched_ok(12, 31, 1) == 0
    assert bc.bc_sched_ok(12, 60, 2 ** 40 + 1) == 0
    # the replay never accepts what the pointwise kernel's own replay rejects
    for k in range(32, 61):
        for c in (1, 2 ** 10 + 1, 2 ** 14 - 1, 2 ** 20 + 1, 2 ** (k - 26) + 1, 2 ** 31 - 1):
            if bc.bc_sched_ok(12, k, c):
                assert bc.split_sched_ok(12, k, c), (k, c)


@pytest.mark.parametrize("bits", [47, 52, 57])
def test_bit_sweep_base_case_or_fallback(bc, oracle, bits):
    """A 4096-point NTT prime of each width either takes the base case (and is exact) or is refused by the replay."""
    n = 4096
    q = ntt_prime_below(2 ** bits, n)
    g = next(x for x in range(2, 200) if pow(x, (q - 1) // 2, q) == q - 1)
    psi = pow(g, (q - 1) // (2 * n), q)
    rng = np.random.default_rng(bits)
    a = rng.integers(0, q, (2, n), dtype=np.uint64); b = rng.integers(0, q, (2, n), dtype=np.uint64)
    a[1] = q - 1; b[1] = q - 1
    if bc.bc_enabled(n, q, psi):
        assert np.array_equal(polymul(bc, n, q, psi, a, b), oracle.poly_mult(a, b, q, psi))
    else:
        c = np.empty_like(a)
        assert bc.bc_polymul(n, q, psi, p64(a), p64(b), p64(c), 2, 0) == -1
