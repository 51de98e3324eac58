"""GPU tests of the prepared dot product (tn_poly_dot_prepared_dev through Plan.poly_dot_prepared): exact equality with the sum
mod q of the three-transform fused products, with the oracle and with the CPU stepping."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_dot_emu import EmuDot, sum_mod, term_rows
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


def device_sum(plan, a3, b3):
    """Sum mod q over the terms of plan.poly_mult(a[:, j], b[:, j], variant="fused"): device tensors (batch, terms, n)."""
    import torch
    acc = None
    for j in range(a3.shape[1]):
        p = plan.poly_mult(a3[:, j].contiguous(), b3[:, j].contiguous(), variant="fused")
        if acc is None:
            acc = p
        else:                                   # canonical words: the sum is below 2q < 2^63 / 2^32; in a 32-bit lane it shows as
            acc = acc + p                       # negative from 2^31 on (q > 2^30), which is above q, and - q wraps it back
            acc = torch.where((acc < 0) | (acc >= plan.q), acc - plan.q, acc)
    return acc


def check_parity(plan, dot, oracle, n, q, psi, a, b, canonical):
    assert plan.has_fused
    a, b = np.array(a), np.array(b)               # (the shared rows are read-only; torch wants writable memory to wrap)
    batch = 5
    for terms in (2, 3):
        idx = term_rows(batch, terms)
        flat = idx.ravel()
        a3 = a[idx]                               # (batch, terms, n)
        for shared in (False, True):
            bidx = np.tile(np.arange(terms), batch) if shared else flat
            prepared = plan.prepare(b[:terms] if shared else b[flat])
            assert prepared.rows == (terms if shared else batch * terms)
            c = plan.poly_dot_prepared(a3, prepared).astype(np.uint64)
            assert c.shape == (batch, n)
            da, db = plan.to_device(a[flat]).reshape(batch, terms, n), plan.to_device(b[bidx]).reshape(batch, terms, n)
            assert np.array_equal(c, plan.to_host(device_sum(plan, da, db)).astype(np.uint64)), (terms, shared)
            ref = sum_mod(oracle.poly_mult(a[flat], b[bidx], q, psi).reshape(batch, terms, n), q)
            assert np.array_equal(c, ref), (terms, shared)
            bhat = plan.to_host(prepared.tensor).astype(np.uint64)
            assert np.array_equal(c, dot.poly_dot_prepared(n, q, psi, a3, bhat, canonical)), (terms, shared)
            # a device tensor in, a device tensor out
            import torch
            dc = plan.poly_dot_prepared(da, prepared)
            assert dc.shape == (batch, n) and torch.equal(dc, plan.to_device(c.astype(plan.dtype)))
    # one output polynomial: (terms, n) in, (n,) out
    one = plan.poly_dot_prepared(a[:3], plan.prepare(b[:3])).astype(np.uint64)
    assert one.shape == (n,)
    assert np.array_equal(one, sum_mod(oracle.poly_mult(a[:3], b[:3], q, psi)[None], q)[0])
    # terms = 1 is the prepared product
    prepared = plan.prepare(b)
    c1 = plan.poly_dot_prepared(a[:, None, :], prepared).astype(np.uint64)
    assert np.array_equal(c1, plan.poly_mult_prepared(a, prepared).astype(np.uint64))
    shared1 = plan.prepare(b[:1])
    assert np.array_equal(plan.poly_dot_prepared(a[:, None, :], shared1), plan.poly_mult_prepared(a, shared1))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_dot_product_equals_summed_fused_products_oracle_and_stepping(eng, dot, oracle, case):
    n, q, psi, a, b = _case_data(case)
    check_parity(eng.get_plan(n, q, psi), dot, oracle, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_dot_product_on_a_canonical_policy_plan(eng, dot, oracle, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(plan, dot, oracle, n, q, psi, a, b, True)


def test_opposite_terms_cancel_and_the_sum_wraps(eng, oracle):
    """terms = 2 with a[r][1] = -a[r][0] and one b: all zeros.  terms = 7 with every word q - 1: wraps mod q on every term."""
    n, q, psi, a, b = _case_data("P4096_60")
    plan = eng.get_plan(n, q, psi)
    a0 = np.array(a[:3])
    a1 = (np.uint64(q) - a0 % np.uint64(q)) % np.uint64(q)
    pair = np.stack([a0, a1], axis=1)
    assert not plan.poly_dot_prepared(pair, plan.prepare(np.array(b[[0, 0]]))).any()
    assert not plan.poly_dot_prepared(pair, plan.prepare(np.array(b[[0, 0, 1, 1, 2, 2]]))).any()
    terms = 7
    ones = np.full((1, n), q - 1, dtype=np.uint64)
    one = oracle.poly_mult(ones, ones, q, psi)
    assert int(one[0, 0]) == q - (n - 2)
    ref = np.repeat(sum_mod(np.repeat(one[:, None, :], terms, axis=1), q), 2, axis=0)
    full = np.full((2, terms, n), q - 1, dtype=np.uint64)
    assert np.array_equal(plan.poly_dot_prepared(full, plan.prepare(np.repeat(ones, terms, axis=0))).astype(np.uint64), ref)
    assert np.array_equal(plan.poly_dot_prepared(full, plan.prepare(np.repeat(ones, 2 * terms, axis=0))).astype(np.uint64), ref)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_small_and_large_batches(eng, tag):
    """terms = 2 at batch 1, 7 and a batch above any grid of resident workgroups (16 workgroups of two waves, 4 of eight waves
    per CU at the most): two launches agree with each other and with the summed products, and leave the prepared rows alone."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (16 if n == 1024 else 4) * cus + 5
    terms = 2
    b_set = plan.fill_lcg(terms, 77, 2)
    shared = plan.prepare(b_set)
    b_all = plan.fill_lcg(big * terms, 2, 2)
    per_set = plan.prepare(b_all)
    before = shared.tensor.clone(), per_set.tensor.clone()
    a_all = plan.fill_lcg(big * terms, 1, 2)
    for batch in (1, 7, big):
        a3 = a_all[:batch * terms].reshape(batch, terms, n)
        for prepared, b3 in ((shared, b_set.expand(batch, terms, n)), (per_set, b_all[:batch * terms].reshape(batch, terms, n))):
            if prepared is per_set:
                prepared = eng.PreparedOperand(plan, per_set.tensor[:batch * terms], batch * terms)
            c1 = plan.poly_dot_prepared(a3, prepared)
            c2 = plan.poly_dot_prepared(a3, prepared)
            assert torch.equal(c1, device_sum(plan, a3, b3)), (tag, batch)
            assert torch.equal(c1, c2), (tag, batch)
    assert torch.equal(shared.tensor, before[0]) and torch.equal(per_set.tensor, before[1])


def test_dynamic_row_hand_out(eng, emu, oracle):
    """Enough output rows at n = 4096 / 60-bit, terms = 2 for plan_rows to hand rows out through the device counter: the
    smallest batch that launch_plan.h's plan_rows calls dynamic for this kernel's row size (terms * n * 8 bytes) when 4
    workgroups per CU are resident, which is above what any fused kernel of this size reaches."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms = 2
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = smallest_dynamic_batch(terms * n * plan.elem_bytes, resident)
    a = plan.fill_lcg(rows * terms, 1, 2); b = plan.fill_lcg(rows * terms, 2, 2)
    a3, b3 = a.reshape(rows, terms, n), b.reshape(rows, terms, n)
    c = plan.poly_dot_prepared(a3, plan.prepare(b))
    assert torch.equal(c, device_sum(plan, a3, b3))
    c_shared = plan.poly_dot_prepared(a3, plan.prepare(b[:terms]))
    assert torch.equal(c_shared, device_sum(plan, a3, b[:terms].expand(rows, terms, n)))
    idx = [0, 1, 511, 512, 1777, 3071, 3072, rows - 1]
    sel = torch.tensor(idx, device=a.device)
    ha = plan.to_host(a3[sel].reshape(-1, n)); hb = plan.to_host(b3[sel].reshape(-1, n))
    ref = sum_mod(oracle.poly_mult(ha, hb, q, psi).reshape(len(idx), terms, n), q)
    assert np.array_equal(plan.to_host(c[sel]).astype(np.uint64), ref)
    hb0 = np.tile(plan.to_host(b[:terms]), (len(idx), 1))
    ref = sum_mod(oracle.poly_mult(ha, hb0, q, psi).reshape(len(idx), terms, n), q)
    assert np.array_equal(plan.to_host(c_shared[sel]).astype(np.uint64), ref)


def test_launch_on_a_side_stream(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms = 3
    a = plan.fill_lcg(9 * terms, 5, 2); b = plan.fill_lcg(9 * terms, 6, 2)
    a3, b3 = a.reshape(9, terms, n), b.reshape(9, terms, n)
    ref = device_sum(plan, a3, b3)
    ref_shared = device_sum(plan, a3, b[:terms].expand(9, terms, n))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = plan.poly_dot_prepared(a3, plan.prepare(b, stream=side), stream=side)
        c_shared = plan.poly_dot_prepared(a3, plan.prepare(b[:terms]))          # stream=None: torch's current stream, `side` here
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c_shared, ref_shared)


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, terms = 5, 2
    a = plan.fill_lcg(batch * terms, 1, 2); b = plan.fill_lcg(batch * terms, 2, 2)
    a3, b3 = a.reshape(batch, terms, n), b.reshape(batch, terms, n)
    prepared = plan.prepare(b)
    c = torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, BH, C = a.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr()
    row_bytes = n * plan.elem_bytes

    def dotp(p, a_, bh, sets, c_, batch_, terms_):
        return lib.tn_poly_dot_prepared_dev(p._h, a_, bh, sets, c_, batch_, terms_, stream)

    assert dotp(plan, A, BH, batch, C, batch, terms) == eng.TN_OK
    assert lib.tn_poly_dot_prepared_dev(None, A, BH, batch, C, batch, terms, stream) == eng.TN_EINVAL             # NULL plan
    assert dotp(plan, None, BH, batch, C, batch, terms) == eng.TN_EINVAL
    assert dotp(plan, A, None, batch, C, batch, terms) == eng.TN_EINVAL
    assert dotp(plan, A, BH, batch, None, batch, terms) == eng.TN_EINVAL
    assert dotp(plan, A, BH, batch, C, batch, 0) == eng.TN_EINVAL                                                  # terms == 0
    assert dotp(plan, A, BH, 2, C, batch, terms) == eng.TN_EINVAL                                                  # neither 1 nor batch
    assert dotp(plan, A, BH, batch, A, batch, terms) == eng.TN_EINVAL                                              # c is a
    assert dotp(plan, A, BH, batch, BH, batch, terms) == eng.TN_EINVAL                                             # c is bhat
    # c's first row is the last of a's batch * terms rows / the last row of the shared set
    assert dotp(plan, A, BH, batch, A + (batch * terms - 1) * row_bytes, batch, terms) == eng.TN_EINVAL
    assert dotp(plan, A, BH, 1, BH + (terms - 1) * row_bytes, batch, terms) == eng.TN_EINVAL
    # c's last row is the first row of a / of the shared set
    assert dotp(plan, A, BH, batch, A - (batch - 1) * row_bytes, batch, terms) == eng.TN_EINVAL
    assert dotp(plan, A, BH, 1, BH - (batch - 1) * row_bytes, batch, terms) == eng.TN_EINVAL
    # just past the shared set is fine for the overlap check of a shared launch: row `terms` of bhat is not part of it
    assert dotp(plan, A, BH, 1, BH + terms * row_bytes, 1, terms) == eng.TN_OK
    # batch * terms = 2^31: refused before anything is launched (dummy non-NULL pointers)
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_terms in ((2 ** 31, 1), (2 ** 30, 2), (1, 2 ** 31), (2 ** 16, 2 ** 15), (3, 2 ** 63)):
        assert dotp(plan, dummy, dummy, 1, dummy, big_batch, big_terms) == eng.TN_EINVAL, (big_batch, big_terms)
    assert dotp(plan, None, None, 1, None, 0, 3) == eng.TN_OK                                                      # batch 0 launches nothing
    torch.cuda.synchronize()
    assert torch.equal(c, device_sum(plan, a3, b3))

    # plans without the fused kernels: a general plan, an omega-only plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    for other in others:
        assert not other.has_fused
        x = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty_like(x); z = torch.empty_like(x[:2])
        assert dotp(other, x.data_ptr(), y.data_ptr(), 2, z.data_ptr(), 2, 2) == eng.TN_EUNSUPPORTED

    # the Python side: a prepared operand is tied to the plan that made it and comes from Plan.prepare
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_dot_prepared(a3, prepared)
    with pytest.raises(TypeError):
        plan.poly_dot_prepared(a3, b)
    with pytest.raises(ValueError):
        plan.poly_dot_prepared(a3, plan.prepare(b[:3]))                  # 3 rows: neither terms nor batch * terms
