"""GPU tests of tn_poly_blind_rotate_prepared_dev at the policy-boundary moduli of tests/policy_moduli.py (its QUICK subset,
which holds every boundary pair of n = 4096: the last modulus the base case accepts and the first it refuses among them), on
the plan the library picks and, where that is lazy, on the forced-canonical plan.  Batch 7, two steps (step 0 with the
exponents of tests/test_cmux_emu.py), every (terms, w) of gadget_pairs, both digit modes: against the loop on the device
(Plan.blind_rotate) and, for one pair, against the CPU stepping of the kernel."""

import numpy as np
import pytest

from policy_moduli import QUICK, entry_id, psi_of
from test_blindrot_emu import BATCH, EmuBlindrot, step_exponents, step_key_rows
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_gpu_blindrot import dev_exps
from test_prepared_emu import operand_rows

pytestmark = pytest.mark.gpu
STEPS = 2


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def blindrot():
    return EmuBlindrot()


def check_entry(plan, blindrot, n, q, psi):
    import torch
    a, b = operand_rows(n, q, n + q % 1000)
    exps = step_exponents(n, STEPS)
    de = dev_exps(exps)
    for t, (terms, w) in enumerate(gadget_pairs(q)):
        ha = np.ascontiguousarray(a[input_rows(BATCH, 2, t)])             # (7, 2, n): every row of the case in every launch
        da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
        keys = plan.prepare(b[step_key_rows(STEPS, terms).ravel()])
        for balanced in MODES:
            where = (n, q, plan.is_lazy, terms, w, balanced)
            c = plan.poly_blind_rotate_prepared(da, de, keys, terms, w, balanced)
            assert torch.equal(c, plan.blind_rotate(da, de, keys, terms, w, balanced)), where
            if t == 0:
                hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
                bhat = plan.to_host(keys.tensor).astype(np.uint64)
                assert np.array_equal(hc, blindrot.rotate(n, q, psi, ha, exps, bhat, terms, w, balanced, not plan.is_lazy)), where


@pytest.mark.parametrize("entry", QUICK, ids=[entry_id(e) for e in QUICK])
def test_blind_rotation_at_policy_boundary_moduli(eng, blindrot, entry):
    """One case per modulus: the plan the library picks, and for a lazy one the forced-canonical plan too."""
    n, q, lazy, bc = entry
    psi = psi_of(n, q)
    for flags in ((0, eng.PLAN_FORCE_CANONICAL) if lazy else (0,)):
        plan = eng.Plan(n, q, psi, 0, flags)
        try:
            assert plan.has_fused and plan.is_lazy == (lazy and flags == 0), (n, q, flags)
            if blindrot.lds(n, plan.elem_bytes, plan.is_lazy)[0]:
                check_entry(plan, blindrot, n, q, psi)
                continue
            # n = 8192 with 64-bit words: the accumulator does not fit, the call says so and names the loop
            assert (n, plan.elem_bytes) == (8192, 8)
            a, b = operand_rows(n, q, n + q % 1000)
            da = plan.to_device(a[:4]).reshape(2, 2, n)
            with pytest.raises(eng.TinyNttError, match="tn_poly_cmux_rotate_prepared_dev"):
                plan.poly_blind_rotate_prepared(da, dev_exps(step_exponents(n, 1, 2)), plan.prepare(b[step_key_rows(1, 2).ravel()]), 2, 31)
        finally:
            plan.close()
