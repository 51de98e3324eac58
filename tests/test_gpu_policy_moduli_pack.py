"""GPU tests of tn_poly_pack_step_prepared_dev at the policy-boundary moduli of tests/policy_moduli.py (its QUICK subset, which holds
every boundary pair of n = 4096: the last modulus the base case accepts and the first it refuses among them), on the plan the
library picks and, where that is lazy, on the forced-canonical plan.  Batch 7, every (terms, w) of gadget_pairs, the Galois
elements and rotations of tests/test_pack_emu.py in turn, every other launch followed by the trace step: against the explicit
route on the device and against the numpy statements of X^rot and sigma_g with the oracle's summed products of the
Python-decomposed digits."""

import numpy as np
import pytest

from policy_moduli import QUICK, entry_id, psi_of
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_galoisks_emu import key_rows
from test_gpu_pack import dev, explicit, host
from test_pack_emu import BATCH, elements, rotations
from test_policy_moduli_pack_emu import oracle_route
from test_prepared_emu import operand_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


def check_entry(eng, plan, oracle, n, q, psi):
    import torch
    a, b = operand_rows(n, q, n + q % 1000)
    gs, rots = elements(n), rotations(n)
    turn = 0
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        hev = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])            # (7, 2, n): every row of the case in every launch
        hod = np.ascontiguousarray(b[input_rows(BATCH, 2, t + 1)])
        ev, od = dev(plan, hev), dev(plan, hod)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
            for balanced in MODES:
                g, rot = gs[turn % len(gs)], rots[turn % len(rots)]
                for o, ho, r in (((od, hod, rot), (None, None, 0)) if turn % 2 == 0 else ((od, hod, rot),)):
                    where = (n, q, plan.is_lazy, terms, w, shared, balanced, g, r, o is None)
                    c = plan.poly_pack_step_prepared(ev, o, r, g, prepared, terms, w, balanced)
                    assert torch.equal(c, explicit(plan, ev, o, r, g, prepared, terms, w, balanced)), where
                    assert np.array_equal(host(plan, c), oracle_route(oracle, n, q, psi, hev, ho, r, g, b, idx, terms, w, balanced)), where
                turn += 1


@pytest.mark.parametrize("entry", QUICK, ids=[entry_id(e) for e in QUICK])
def test_pack_step_at_policy_boundary_moduli(eng, oracle, entry):
    """One case per modulus: the plan the library picks, and for a lazy one the forced-canonical plan too."""
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    for flags in ((0, eng.PLAN_FORCE_CANONICAL) if lazy else (0,)):
        plan = eng.Plan(n, q, psi, 0, flags)
        try:
            assert plan.has_fused and plan.is_lazy == (lazy and flags == 0), (n, q, flags)
            check_entry(eng, plan, oracle, n, q, psi)
        finally:
            plan.close()
