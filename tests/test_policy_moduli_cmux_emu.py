"""CPU stepping of the CMux rotation kernel (tests/emu/emu_cmux.cpp) at the policy-boundary moduli of tests/policy_moduli.py, the full
table: the last prime each bound schedule accepts and the first it refuses, among them the last modulus the base case accepts
and the first it refuses at n = 4096; lazy plans and, where lazy, forced-canonical plans.  Batch 7 with the exponents of
tests/test_cmux_emu.py, every (terms, w) of gadget_pairs: against the numpy statement of the definition (the monomial in
numpy, the stepping of the external-product kernel, the addition) and against the oracle's summed products of the
Python-decomposed digits."""
import numpy as np
import pytest

from policy_moduli import ENTRIES, entry_id, psi_of, sum_terms
from test_cmux_emu import BATCH, EmuCmux, definition, exponents, key_rows
from test_extprod_emu import EmuExtprod, digit_rows, input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_prepared_emu import EmuPrepared, operand_rows

RUNS = [(e, canonical) for e in ENTRIES for canonical in ((False, True) if e[2] else (True,))]
RUN_IDS = [entry_id(e) + ("_canonical" if canonical else "") for e, canonical in RUNS]


@pytest.fixture(scope="module")
def cmux():
    return EmuCmux()


@pytest.fixture(scope="module")
def extprod():
    return EmuExtprod()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_rotation_matches_the_definition_and_the_oracle(cmux, extprod, prep, oracle, entry, canonical):
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    a, b = operand_rows(n, q, n + q % 1000)
    bhat = prep.prepare(n, q, psi, b, canonical)
    exps = exponents(n)
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        a7 = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        # a shared key and a key per row for every pair, each digit mode with both over two consecutive pairs (the full
        # product of key and mode at every pair is tests/test_cmux_emu.py's, on its shapes)
        for shared, balanced in (((True, MODES[0]), (False, MODES[1])) if t % 2 == 0 else ((True, MODES[1]), (False, MODES[0]))):
            where = (n, q, canonical, terms, w, shared, balanced)
            idx = key_rows(BATCH, terms, shared)
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            c = cmux.rotate(n, q, psi, a7, exps, bh, terms, w, balanced, canonical)
            m, ref = definition(extprod, n, q, psi, a7, exps, bh, terms, w, balanced, canonical)
            assert np.array_equal(c, ref), where
            digits = digit_rows(m, q, w, terms, balanced)
            for o in range(2):
                prods = oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(BATCH, 2 * terms, n)
                assert np.array_equal(c[:, o], (a7[:, o] % np.uint64(q) + sum_terms(prods, q)) % np.uint64(q)), where + (o,)
