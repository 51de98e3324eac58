"""CPU stepping of the pack / trace step kernel (tests/emu_pack/emu_pack.cpp) at the policy-boundary moduli of tests/policy_moduli.py,
the full table: the last prime each bound schedule accepts and the first it refuses, among them the last modulus the base case
accepts and the first it refuses at n = 4096; lazy plans and, where lazy, forced-canonical plans.  Batch 7, every (terms, w) of
gadget_pairs, the Galois elements and rotations of tests/test_pack_emu.py in turn, and the trace step: against the stepped explicit
route and against the numpy statements of X^rot and sigma_g with the oracle's summed products of the Python-decomposed digits."""
import numpy as np
import pytest

from policy_moduli import ENTRIES, entry_id, psi_of
from test_cmux_emu import EmuCmux, monomial_np
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_galoisks_emu import EmuGaloisKs, key_rows
from test_pack_emu import BATCH, EmuPack, elements, rotations, stepped_route, sum_and_difference
from test_policy_moduli_galoisks_emu import oracle_route as galoisks_oracle_route
from test_prepared_emu import EmuPrepared, operand_rows

RUNS = [(e, canonical) for e in ENTRIES for canonical in ((False, True) if e[2] else (True,))]
RUN_IDS = [entry_id(e) + ("_canonical" if canonical else "") for e, canonical in RUNS]


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


def oracle_route(oracle, n, q, psi, ev, od, rot, g, b, idx, terms, w, balanced):
    """X^rot in numpy, s and d in numpy, the automorphism key switch of d by the numpy sigma_g, the Python decomposition and the
    oracle's summed products (tests/test_policy_moduli_galoisks_emu.py), s added: (batch, 2, n)."""
    t = np.zeros_like(ev) if od is None else monomial_np(od, np.full(ev.shape[0], rot), q)
    s, d = sum_and_difference(ev, t, q)
    return (galoisks_oracle_route(oracle, n, q, psi, d, g, b, idx, terms, w, balanced) + s) % np.uint64(q)


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_pack_step_matches_the_route_and_the_oracle(pack, ks, cmux, prep, oracle, entry, canonical):
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    a, b = operand_rows(n, q, n + q % 1000)
    bhat = prep.prepare(n, q, psi, b, canonical)
    gs, rots = elements(n), rotations(n)
    turn = 0
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        ev = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        od = np.ascontiguousarray(b[input_rows(BATCH, 2, t + 1)])
        # a shared key and a key per row for every pair, each digit mode with both over two consecutive pairs, the elements and
        # rotations in turn, every other launch followed by the trace step (the full product is tests/test_pack_emu.py's)
        for shared, balanced in (((True, MODES[0]), (False, MODES[1])) if t % 2 == 0 else ((True, MODES[1]), (False, MODES[0]))):
            g, rot = gs[turn % len(gs)], rots[turn % len(rots)]
            idx = key_rows(BATCH, terms, shared)
            bh = bhat[idx[0].ravel()] if shared else bhat[idx.ravel()]
            for o, r in (((od, rot), (None, 0)) if turn % 2 == 0 else ((od, rot),)):
                where = (n, q, canonical, terms, w, shared, balanced, g, r, o is None)
                c = pack.step(n, q, psi, ev, o, r, g, bh, terms, w, balanced, canonical)
                assert np.array_equal(c, stepped_route(ks, cmux, n, q, psi, ev, o, r, g, bh, terms, w, balanced, canonical)), where
                assert np.array_equal(c, oracle_route(oracle, n, q, psi, ev, o, r, g, b, idx, terms, w, balanced)), where
            turn += 1
