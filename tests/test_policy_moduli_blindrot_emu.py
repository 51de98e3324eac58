"""CPU stepping of the blind-rotation kernel (tests/emu/emu_blindrot.cpp) at the policy-boundary moduli of tests/policy_moduli.py, the
full table: the last prime each bound schedule accepts and the first it refuses, among them the last modulus the base case
accepts and the first it refuses at n = 4096; lazy plans and, where lazy, forced-canonical plans.  Batch 7, two steps (step 0
with the exponents of tests/test_cmux_emu.py), every (terms, w) of gadget_pairs with the digit modes alternating over the
pairs: against the loop of stepped CMux rotations (tests/emu/emu_cmux.cpp) on the steps' shared keys.  A shape the LDS rule refuses is
refused by the stepping."""
import numpy as np
import pytest

from policy_moduli import ENTRIES, entry_id, psi_of
from test_blindrot_emu import BATCH, EmuBlindrot, loop_of_steps, step_exponents, step_key_rows
from test_cmux_emu import EmuCmux
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_prepared_emu import EmuPrepared, operand_rows

STEPS = 2
RUNS = [(e, canonical) for e in ENTRIES for canonical in ((False, True) if e[2] else (True,))]
RUN_IDS = [entry_id(e) + ("_canonical" if canonical else "") for e, canonical in RUNS]


@pytest.fixture(scope="module")
def blindrot():
    return EmuBlindrot()


@pytest.fixture(scope="module")
def cmux():
    return EmuCmux()


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


@pytest.mark.parametrize("entry,canonical", RUNS, ids=RUN_IDS)
def test_blind_rotation_is_the_loop_of_rotations(blindrot, cmux, prep, entry, canonical):
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    a, b = operand_rows(n, q, n + q % 1000)
    exps = step_exponents(n, STEPS)
    if not blindrot.lds(n, 4 if q < 2 ** 31 else 8, not canonical)[0]:
        rc, _ = blindrot.rotate_code(n, q, psi, a[input_rows(1, 2)], exps[:1, :1], np.zeros((4, n), dtype=np.uint64), 1, 1, False, canonical)
        assert rc == 8
        return
    bhat = prep.prepare(n, q, psi, b, canonical)
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        a7 = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        balanced = MODES[t % 2]                                           # each digit mode over two of the four pairs
        bh = bhat[step_key_rows(STEPS, terms).ravel()]
        ref = loop_of_steps(cmux, n, q, psi, a7, exps, bh, terms, w, balanced, canonical)[-1]
        assert np.array_equal(blindrot.rotate(n, q, psi, a7, exps, bh, terms, w, balanced, canonical), ref), (n, q, canonical, terms, w, balanced)
