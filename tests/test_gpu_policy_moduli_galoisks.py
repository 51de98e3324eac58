"""GPU tests of tn_poly_galois_keyswitch_prepared_dev at the policy-boundary moduli of tests/policy_moduli.py (its QUICK subset,
which holds every boundary pair of n = 4096: the last modulus the base case accepts and the first it refuses among them), on the
plan the library picks and, where that is lazy, on the forced-canonical plan.  Batch 7, every (terms, w) of gadget_pairs, the
seven Galois elements of tests/test_galoisks_emu.py in turn: against the explicit route on the device and against the numpy
statement of sigma_g with the oracle's summed products of the Python-decomposed digits."""

import numpy as np
import pytest

from policy_moduli import QUICK, entry_id, psi_of
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_galoisks_emu import BATCH, elements, key_rows
from test_gpu_galoisks import explicit
from test_policy_moduli_galoisks_emu import oracle_route
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
    gs = elements(n)
    turn = 0
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        ha = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
            for balanced in MODES:
                g = gs[turn % len(gs)]
                turn += 1
                where = (n, q, plan.is_lazy, terms, w, shared, balanced, g)
                c = plan.poly_galois_keyswitch_prepared(da, g, prepared, terms, w, balanced)
                assert torch.equal(c, explicit(plan, da, g, prepared, terms, w, balanced)), where
                hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
                assert np.array_equal(hc, oracle_route(oracle, n, q, psi, ha, g, b, idx, terms, w, balanced)), where


@pytest.mark.parametrize("entry", QUICK, ids=[entry_id(e) for e in QUICK])
def test_key_switch_at_policy_boundary_moduli(eng, oracle, entry):
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
