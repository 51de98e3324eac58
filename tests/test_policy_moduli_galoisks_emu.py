"""CPU stepping of the automorphism key-switch kernel (tests/emu_galoisks/emu_galoisks.cpp) at the policy-boundary moduli of
tests/policy_moduli.py, the full table: the last prime each bound schedule accepts and the first it refuses, among them the last
modulus the base case accepts and the first it refuses at n = 4096; lazy plans and, where lazy, forced-canonical plans.  Batch 7,
every (terms, w) of gadget_pairs, the seven Galois elements of tests/test_galoisks_emu.py in turn: against the stepped explicit
route and against the numpy statement of sigma_g with the oracle's summed products of the Python-decomposed digits."""
import numpy as np
import pytest

from policy_moduli import ENTRIES, entry_id, psi_of, sum_terms
from test_extprod_emu import digit_rows, input_rows
from test_gadget2_emu import EmuGadget2
from test_gadget_emu import MODES, gadget_pairs
from test_galois_emu import EmuGalois, sigma
from test_galoisks_emu import BATCH, EmuGaloisKs, elements, key_rows, stepped_route
from test_prepared_emu import EmuPrepared, operand_rows

RUNS = [(e, canonical) for e in ENTRIES for canonical in ((False, True) if e[2] else (True,))]
RUN_IDS = [entry_id(e) + ("_canonical" if canonical else "") for e, canonical in RUNS]


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


def oracle_route(oracle, n, q, psi, a, g, b, idx, terms, w, balanced):
    """sigma_g in numpy, the Python decomposition of sigma_g(a1), the oracle's products summed, sigma_g(a0) added: (batch, 2, n)."""
    batch = a.shape[0]
    s = sigma(a, g, q)
    digits = digit_rows(np.ascontiguousarray(s[:, 1:2]), q, w, terms, balanced)          # (batch, terms, n)
    out = np.empty((batch, 2, n), dtype=np.uint64)
    for o in range(2):
        prods = oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(batch, terms, n)
        out[:, o] = sum_terms(prods, q)
    out[:, 0] = (out[:, 0] + s[:, 0]) % np.uint64(q)
    return out


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_key_switch_matches_the_route_and_the_oracle(ks, gal, gadget2, prep, oracle, entry, canonical):
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    a, b = operand_rows(n, q, n + q % 1000)
    bhat = prep.prepare(n, q, psi, b, canonical)
    gs = elements(n)
    turn = 0
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        a7 = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        # a shared key and a key per row for every pair, each digit mode with both over two consecutive pairs, the seven elements
        # in turn over the eight launches (the full product is tests/test_galoisks_emu.py's, on its shapes)
        for shared, balanced in (((True, MODES[0]), (False, MODES[1])) if t % 2 == 0 else ((True, MODES[1]), (False, MODES[0]))):
            g = gs[turn % len(gs)]
            turn += 1
            where = (n, q, canonical, terms, w, shared, balanced, g)
            idx = key_rows(BATCH, terms, shared)
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            c = ks.keyswitch(n, q, psi, a7, g, bh, terms, w, balanced, canonical)
            assert np.array_equal(c, stepped_route(gal, gadget2, n, q, psi, a7, g, bh, terms, w, balanced, canonical)), where
            assert np.array_equal(c, oracle_route(oracle, n, q, psi, a7, g, b, idx, terms, w, balanced)), where
