"""GPU tests of the prepared-operand product (tn_prepare_dev / tn_poly_mult_prepared_dev through Plan.prepare /
Plan.poly_mult_prepared): exact equality with the three-transform fused product, the oracle and the CPU stepping."""

import numpy as np
import pytest

from conftest import PARAMS, ntt_prime_below
from test_prepared_emu import CASES, CASE_IDS, EmuPrepared, _case_data, operand_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


def check_parity(plan, prep, oracle, n, q, psi, a, b, canonical):
    assert plan.has_fused
    a, b = np.array(a), np.array(b)               # (the shared rows are read-only; torch wants writable memory to wrap)
    prepared = plan.prepare(b)
    assert prepared.rows == 5 and prepared.plan is plan
    c = plan.poly_mult_prepared(a, prepared).astype(np.uint64)
    assert np.array_equal(c, plan.poly_mult(a, b, variant="fused").astype(np.uint64))
    assert np.array_equal(c, oracle.poly_mult(a, b, q, psi))
    bhat = plan.to_host(prepared.tensor).astype(np.uint64)
    assert np.array_equal(bhat, prep.prepare(n, q, psi, b, canonical))         # word for word: same values, same order
    # one polynomial in, one polynomial out; the prepared row shared by every row of a
    one = plan.prepare(b[4])
    assert one.rows == 1
    assert np.array_equal(plan.poly_mult_prepared(a[4], one).astype(np.uint64), c[4])
    shared = plan.poly_mult_prepared(a, plan.prepare(b[:1])).astype(np.uint64)
    assert np.array_equal(shared, oracle.poly_mult(a, np.repeat(b[:1], 5, axis=0), q, psi))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_prepared_product_equals_fused_product_oracle_and_stepping(eng, prep, oracle, case):
    n, q, psi, a, b = _case_data(case)
    check_parity(eng.get_plan(n, q, psi), prep, oracle, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_prepared_product_on_a_canonical_policy_plan(eng, prep, oracle, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(plan, prep, oracle, n, q, psi, a, b, True)


def test_prepared_product_generic_modulus(eng, prep, oracle):
    from tiny_ntt_amd import numtheory
    n = 1024
    q = ntt_prime_below(2 ** 61, n)
    psi = numtheory.primitive_2n_root(n, q)
    plan = eng.get_plan(n, q, psi)
    assert not plan.is_lazy
    a, b = operand_rows(n, q, 61)
    check_parity(plan, prep, oracle, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_shared_operand_small_and_large_batches(eng, tag):
    """bhat_rows = 1 at batch 1, 7 and a batch above any grid of resident workgroups (16 workgroups of two waves, 4 of eight
    waves per CU at the most): every row is multiplied by the same b, which the launches leave untouched."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (16 if n == 1024 else 4) * cus + 5
    b = plan.fill_lcg(1, 77, 2)
    prepared = plan.prepare(b)
    before = prepared.tensor.clone()
    a_all = plan.fill_lcg(big, 1, 2)
    for batch in (1, 7, big):
        a = a_all[:batch]
        c1 = plan.poly_mult_prepared(a, prepared)
        c2 = plan.poly_mult_prepared(a, prepared)
        ref = plan.poly_mult(a, b.expand(batch, n).contiguous())
        assert torch.equal(c1, ref), (tag, batch)
        assert torch.equal(c1, c2), (tag, batch)
    assert torch.equal(prepared.tensor, before)


def test_dynamic_row_hand_out(eng, oracle):
    """4,096 rows at n = 4096 / 60-bit (128 MiB per buffer): at least 4 rows per resident workgroup, so plan_rows hands rows out
    through the device counter."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    rows = 4096
    a = plan.fill_lcg(rows, 1, 2); b = plan.fill_lcg(rows, 2, 2)
    ref = plan.poly_mult(a, b)
    c = plan.poly_mult_prepared(a, plan.prepare(b))
    assert torch.equal(c, ref)
    ref_shared = plan.poly_mult(a, b[:1].expand(rows, n).contiguous())
    c_shared = plan.poly_mult_prepared(a, plan.prepare(b[:1]))
    assert torch.equal(c_shared, ref_shared)
    idx = [0, 1, 511, 512, 1777, 3071, 3072, rows - 1]
    sel = torch.tensor(idx, device=a.device)
    ha, hb = plan.to_host(a[sel]), plan.to_host(b[sel])
    assert np.array_equal(plan.to_host(c[sel]), oracle.poly_mult(ha, hb, q, psi))
    hb0 = np.repeat(plan.to_host(b[:1]), len(idx), axis=0)
    assert np.array_equal(plan.to_host(c_shared[sel]), oracle.poly_mult(ha, hb0, q, psi))


def test_launch_on_a_side_stream(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    a = plan.fill_lcg(9, 5, 2); b = plan.fill_lcg(9, 6, 2)
    ref = plan.poly_mult(a, b)
    ref_shared = plan.poly_mult(a, b[:1].expand(9, n).contiguous())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        prepared = plan.prepare(b, stream=side)
        c = plan.poly_mult_prepared(a, prepared, stream=side)
        one = plan.prepare(b[:1])                      # stream=None: torch's current stream, which is `side` here
        c_shared = plan.poly_mult_prepared(a, one)
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c_shared, ref_shared)


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    a = plan.fill_lcg(5, 1, 2); b = plan.fill_lcg(5, 2, 2)
    prepared = plan.prepare(b)
    c = torch.empty_like(a)
    stream = plan._stream_ptr(None)

    def mult(p, a_, bh, bh_rows, c_, batch):
        return lib.tn_poly_mult_prepared_dev(p._h, a_, bh, bh_rows, c_, batch, stream)

    assert mult(plan, a.data_ptr(), prepared.tensor.data_ptr(), 5, c.data_ptr(), 5) == eng.TN_OK
    assert mult(plan, a.data_ptr(), prepared.tensor.data_ptr(), 2, c.data_ptr(), 5) == eng.TN_EINVAL          # neither 1 nor batch
    assert mult(plan, a.data_ptr(), prepared.tensor.data_ptr(), 5, prepared.tensor.data_ptr(), 5) == eng.TN_EINVAL      # c is bhat
    row_bytes = n * plan.elem_bytes
    assert mult(plan, a.data_ptr(), prepared.tensor.data_ptr(), 1, prepared.tensor.data_ptr() - 4 * row_bytes, 5) == eng.TN_EINVAL   # c's last row is the shared bhat row
    assert mult(plan, a.data_ptr(), prepared.tensor.data_ptr(), 5, a.data_ptr() + 2 * row_bytes, 3) == eng.TN_EINVAL    # c overlaps a
    assert mult(plan, None, prepared.tensor.data_ptr(), 5, c.data_ptr(), 5) == eng.TN_EINVAL
    assert mult(plan, a.data_ptr(), None, 5, c.data_ptr(), 5) == eng.TN_EINVAL
    assert mult(plan, a.data_ptr(), prepared.tensor.data_ptr(), 5, None, 5) == eng.TN_EINVAL
    assert mult(plan, None, None, 1, None, 0) == eng.TN_OK                                                       # batch 0 launches nothing
    assert lib.tn_prepare_dev(plan._h, None, None, 0, stream) == eng.TN_OK
    assert lib.tn_prepare_dev(plan._h, b.data_ptr(), None, 5, stream) == eng.TN_EINVAL
    assert lib.tn_prepare_dev(plan._h, b.data_ptr(), b.data_ptr() + 4 * row_bytes, 5, stream) == eng.TN_EINVAL    # bhat overlaps b
    torch.cuda.synchronize()
    assert torch.equal(c, plan.poly_mult(a, b))

    # plans without the fused kernels: a general plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    for other in (eng.get_general_plan(n, q, psi), eng.get_plan(16, q, small_psi)):
        assert not other.has_fused
        x = torch.zeros((2, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty_like(x); z = torch.empty_like(x)
        assert lib.tn_prepare_dev(other._h, x.data_ptr(), y.data_ptr(), 2, stream) == eng.TN_EUNSUPPORTED
        assert mult(other, x.data_ptr(), y.data_ptr(), 2, z.data_ptr(), 2) == eng.TN_EUNSUPPORTED
        with pytest.raises(eng.TinyNttError) as e:
            other.prepare(x)
        assert e.value.status == eng.TN_EUNSUPPORTED

    # a prepared operand is tied to the plan that made it
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_mult_prepared(a, prepared)
    with pytest.raises(TypeError):
        plan.poly_mult_prepared(a, b)
