"""GPU tests of tn_poly_cmux_rotate_prepared_dev at the policy-boundary moduli of tests/policy_moduli.py (its QUICK subset, which
holds every boundary pair of n = 4096: the last modulus the base case accepts and the first it refuses among them), on the plan
the library picks and, where that is lazy, on the forced-canonical plan.  Batch 7 with the exponents of tests/test_cmux_emu.py,
every (terms, w) of gadget_pairs: against the explicit route on the device and against the oracle's summed products of the
Python-decomposed digits of the numpy monomial product."""

import numpy as np
import pytest

from policy_moduli import QUICK, entry_id, psi_of, sum_terms
from test_cmux_emu import BATCH, exponents, key_rows, monomial_np
from test_extprod_emu import digit_rows, input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_gpu_cmux import dev_exps, explicit
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
    exps = exponents(n)
    de = dev_exps(exps)
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        ha = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
        m = monomial_np(ha, exps, q, True)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
            for balanced in MODES:
                where = (n, q, plan.is_lazy, terms, w, shared, balanced)
                c = plan.poly_cmux_rotate_prepared(da, de, prepared, terms, w, balanced)
                assert torch.equal(c, explicit(plan, da, de, prepared, terms, w, balanced)), where
                hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
                digits = digit_rows(m, q, w, terms, balanced)
                for o in range(2):
                    prods = oracle.poly_mult(digits.reshape(-1, n), b[idx[:, o].ravel()], q, psi).reshape(BATCH, 2 * terms, n)
                    assert np.array_equal(hc[:, o], (ha[:, o] % np.uint64(q) + sum_terms(prods, q)) % np.uint64(q)), where + (o,)


@pytest.mark.parametrize("entry", QUICK, ids=[entry_id(e) for e in QUICK])
def test_rotation_at_policy_boundary_moduli(eng, oracle, entry):
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
