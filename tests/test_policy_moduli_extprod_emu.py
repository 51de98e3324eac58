"""CPU stepping of the external-product kernel (tests/emu/emu_extprod.cpp) at the policy-boundary moduli of tests/policy_moduli.py, the
full table: the last prime each bound schedule accepts and the first it refuses, among them the last modulus the base case
accepts and the first it refuses at n = 4096; lazy plans and, where lazy, forced-canonical plans.  ins = 2, batch 5, every
(terms, w) of gadget_pairs: against the oracle's summed products of the Python-decomposed digits and against route B (the
stepping of the dot kernel on those digits)."""
import numpy as np
import pytest

from policy_moduli import BC_ENTRIES, ENTRIES, PAIRS, entry_id, psi_of, sum_terms
from test_dot_emu import EmuDot
from test_extprod_emu import EmuExtprod, digit_rows, ext_rows, input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_prepared_emu import EmuPrepared, operand_rows

RUNS = [(e, canonical) for e in ENTRIES for canonical in ((False, True) if e[2] else (True,))]
RUN_IDS = [entry_id(e) + ("_canonical" if canonical else "") for e, canonical in RUNS]
BATCH, INS = 5, 2


@pytest.fixture(scope="module")
def extprod():
    return EmuExtprod()


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def test_table_holds_the_base_case_boundary_at_4096():
    """The last modulus the base case accepts and the first it refuses, per word length, are entries of the table this file runs."""
    pairs = [(first, second) for n, flag, first, second in PAIRS if n == 4096 and flag == "bc"]
    assert len(pairs) >= 4
    table = {(e[0], e[1]): e for e in ENTRIES}
    for first, second in pairs:
        assert table[(4096, first)][3] and not table[(4096, second)][3], (first, second)
    assert {(4096, first) for first, _ in pairs} <= {(e[0], e[1]) for e in BC_ENTRIES}


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_external_product_matches_the_oracle_and_route_b(extprod, dot, prep, oracle, entry, canonical):
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    a, b = operand_rows(n, q, n + q % 1000)
    bhat = prep.prepare(n, q, psi, b, canonical)
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        a5 = a[input_rows(BATCH, INS, t)]                                # (5, 2, n): every row of the case in every launch
        # a shared set and a set per row for every pair, each digit mode with both over two consecutive pairs (the full
        # product of set and mode at every pair is tests/test_extprod_emu.py's, on its shapes)
        for shared, balanced in (((True, MODES[0]), (False, MODES[1])) if t % 2 == 0 else ((True, MODES[1]), (False, MODES[0]))):
            where = (n, q, canonical, terms, w, shared, balanced)
            idx = ext_rows(BATCH, INS, terms)
            if shared:
                idx[1:] = idx[0]
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            c = extprod.external_product(n, q, psi, a5, bh, terms, w, balanced, canonical)
            digits = digit_rows(a5, q, w, terms, balanced)
            for o in range(2):
                bo = bhat[idx[0, o].ravel()] if shared else bhat[idx[:, o].ravel()]
                assert np.array_equal(c[:, o], dot.poly_dot_prepared(n, q, psi, digits, bo, canonical)), where + (o,)
                prods = oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(BATCH, INS * terms, n)
                assert np.array_equal(c[:, o], sum_terms(prods, q)), where + (o,)
