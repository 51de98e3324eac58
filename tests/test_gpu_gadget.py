"""GPU tests of the gadget calls (tn_gadget_decompose_dev and tn_poly_gadget_dot_prepared_dev through Plan.gadget_decompose and
Plan.poly_gadget_dot_prepared): the decomposition against the definition written out in Python, the fused call bit for bit
against tn_poly_dot_prepared_dev on the decomposed rows and against the CPU stepping of its kernel."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_dot_emu import term_rows
from test_gadget_emu import MODES, EmuGadget, decompose_rows, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def gadget():
    return EmuGadget()


def two_launches(plan, a, prepared, terms, w, balanced):
    """The path without the fused call: tn_gadget_decompose_dev, then tn_poly_dot_prepared_dev on its output."""
    return plan.poly_dot_prepared(plan.gadget_decompose(a, terms, w, balanced), prepared)


def check_parity(plan, gadget, n, q, psi, a, b, canonical):
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)               # (the shared rows are read-only; torch wants writable memory to wrap)
    batch = 5
    da = plan.to_device(a)
    for terms, w in gadget_pairs(q):
        for shared in (True, False):
            prepared = plan.prepare(b[:terms] if shared else b[term_rows(batch, terms).ravel()])
            assert prepared.rows == (terms if shared else batch * terms)
            bhat = plan.to_host(prepared.tensor).astype(np.uint64)
            for balanced in MODES:
                where = (terms, w, shared, balanced)
                digits = plan.gadget_decompose(da, terms, w, balanced)
                assert digits.shape == (batch, terms, n)
                assert np.array_equal(plan.to_host(digits.reshape(-1, n)).astype(np.uint64).reshape(batch, terms, n),
                                      decompose_rows(a, q, w, terms, balanced)), where
                c = plan.poly_gadget_dot_prepared(da, prepared, terms, w, balanced)
                assert c.shape == (batch, n)
                assert torch.equal(c, plan.poly_dot_prepared(digits, prepared)), where
                hc = plan.to_host(c).astype(np.uint64)
                assert np.array_equal(hc, gadget.poly_gadget_dot_prepared(n, q, psi, a, bhat, terms, w, balanced, canonical)), where
    # host arrays in, host arrays out; one polynomial: (n,) in, (terms, n) and (n,) out
    terms, w = gadget_pairs(q)[1]
    prepared = plan.prepare(b[:terms])
    hd = plan.gadget_decompose(a, terms, w, True)
    assert isinstance(hd, np.ndarray) and np.array_equal(hd.astype(np.uint64), decompose_rows(a, q, w, terms, True))
    hc = plan.poly_gadget_dot_prepared(a, prepared, terms, w, True)
    assert isinstance(hc, np.ndarray) and np.array_equal(hc, plan.to_host(two_launches(plan, da, prepared, terms, w, True)))
    one = plan.gadget_decompose(a[0], terms, w)
    assert one.shape == (terms, n) and np.array_equal(one.astype(np.uint64), decompose_rows(a[:1], q, w, terms, False)[0])
    one = plan.poly_gadget_dot_prepared(a[2], prepared, terms, w, True)
    assert one.shape == (n,) and np.array_equal(one, hc[2])
    # terms = 1: one digit, then the prepared product
    prepared = plan.prepare(b)
    for balanced in MODES:
        c1 = plan.poly_gadget_dot_prepared(da, prepared, 1, 7, balanced)
        d1 = plan.gadget_decompose(da, 1, 7, balanced)
        assert torch.equal(c1, plan.poly_mult_prepared(d1[:, 0].contiguous(), prepared))
        assert torch.equal(c1, plan.poly_dot_prepared(d1, prepared))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_gadget_product_equals_decompose_then_dot_and_the_stepping(eng, gadget, case):
    n, q, psi, a, b = _case_data(case)
    check_parity(eng.get_plan(n, q, psi), gadget, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_gadget_product_on_a_canonical_policy_plan(eng, gadget, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(plan, gadget, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_small_and_large_batches(eng, tag):
    """terms = 2 at batch 1, 7 and a batch above any grid of resident workgroups (16 workgroups of two waves, 4 of eight waves
    per CU at the most): two launches agree with each other and with decompose + dot, and leave the prepared rows alone."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (16 if n == 1024 else 4) * cus + 5
    terms, w = gadget_pairs(q)[0]
    shared = plan.prepare(plan.fill_lcg(terms, 77, 2))
    per_set = plan.prepare(plan.fill_lcg(big * terms, 2, 2))
    before = shared.tensor.clone(), per_set.tensor.clone()
    a_all = plan.fill_lcg(big, 1, 2)
    for batch in (1, 7, big):
        a = a_all[:batch]
        for prepared in (shared, eng.PreparedOperand(plan, per_set.tensor[:batch * terms], batch * terms)):
            for balanced in MODES:
                c1 = plan.poly_gadget_dot_prepared(a, prepared, terms, w, balanced)
                c2 = plan.poly_gadget_dot_prepared(a, prepared, terms, w, balanced)
                assert torch.equal(c1, two_launches(plan, a, prepared, terms, w, balanced)), (tag, batch, balanced)
                assert torch.equal(c1, c2), (tag, batch, balanced)
    assert torch.equal(shared.tensor, before[0]) and torch.equal(per_set.tensor, before[1])


def test_dynamic_row_hand_out(eng, emu, gadget):
    """Enough output rows at n = 4096 / 60-bit, terms = 2 for plan_rows to hand rows out through the device counter.  The
    launcher plans an output row as the prepared dot product does, with terms * n * 8 bytes (launch_plan.h dot_row_bytes): one
    output row is `terms` forward transforms of work between two atomics although one row of a is read for it.  The batch is
    the smallest that plan_rows calls dynamic for that row size when 4 workgroups per CU are resident, which is above what any
    fused kernel of this size reaches."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w = 2, 30
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = smallest_dynamic_batch(terms * n * plan.elem_bytes, resident)
    a = plan.fill_lcg(rows, 1, 2); b = plan.fill_lcg(rows * terms, 2, 2)
    per_set, shared = plan.prepare(b), plan.prepare(b[:terms])
    digits = plan.gadget_decompose(a, terms, w, True)
    c = plan.poly_gadget_dot_prepared(a, per_set, terms, w, True)
    assert torch.equal(c, plan.poly_dot_prepared(digits, per_set))
    c_shared = plan.poly_gadget_dot_prepared(a, shared, terms, w, True)
    assert torch.equal(c_shared, plan.poly_dot_prepared(digits, shared))
    # a few rows, among them the first and last of the launch and of chunks in between, against the CPU stepping
    idx = [0, 1, 511, 512, 1777, 3071, 3072, rows - 1]
    sel = torch.tensor(idx, device=a.device)
    ha = plan.to_host(a[sel]).astype(np.uint64)
    hb = plan.to_host(per_set.tensor.reshape(rows, terms, n)[sel].reshape(-1, n)).astype(np.uint64)
    assert np.array_equal(plan.to_host(c[sel]).astype(np.uint64), gadget.poly_gadget_dot_prepared(n, q, psi, ha, hb, terms, w, True))


def test_launch_on_a_side_stream(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w = 3, 20
    a = plan.fill_lcg(9, 5, 2); b = plan.fill_lcg(9 * terms, 6, 2)
    per_set, shared = plan.prepare(b), plan.prepare(b[:terms])
    ref = two_launches(plan, a, per_set, terms, w, True)
    ref_shared = two_launches(plan, a, shared, terms, w, False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = plan.poly_gadget_dot_prepared(a, per_set, terms, w, True, stream=side)
        c_shared = plan.poly_gadget_dot_prepared(a, shared, terms, w)           # stream=None: torch's current stream, `side` here
        d = plan.gadget_decompose(a, terms, w, True, stream=side)
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c_shared, ref_shared)
    assert torch.equal(d, plan.gadget_decompose(a, terms, w, True))


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    k = q.bit_length()
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, terms, w = 5, 2, 30
    a = plan.fill_lcg(batch, 1, 2); b = plan.fill_lcg(batch * terms, 2, 2)
    prepared = plan.prepare(b)
    c = torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device)
    d = torch.empty((batch, terms, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, BH, C, D = a.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr(), d.data_ptr()
    row_bytes = n * plan.elem_bytes
    OK, EINVAL = eng.TN_OK, eng.TN_EINVAL

    def dotp(p, a_, bh, sets, c_, batch_, terms_, w_=w, flags=0):
        return lib.tn_poly_gadget_dot_prepared_dev(p._h, a_, bh, sets, c_, batch_, terms_, w_, flags, stream)

    def dec(p, a_, d_, batch_, terms_, w_=w, flags=0):
        return lib.tn_gadget_decompose_dev(p._h, a_, d_, batch_, terms_, w_, flags, stream)

    last = two_launches(plan, a, prepared, terms, k - 1, False)      # what the last accepted launch into c below computes
    assert dotp(plan, A, BH, batch, C, batch, terms) == OK and dec(plan, A, D, batch, terms) == OK
    assert dotp(plan, A, BH, batch, C, batch, terms, w, eng.GADGET_BALANCED) == OK
    assert lib.tn_poly_gadget_dot_prepared_dev(None, A, BH, batch, C, batch, terms, w, 0, stream) == EINVAL      # NULL plan
    assert lib.tn_gadget_decompose_dev(None, A, D, batch, terms, w, 0, stream) == EINVAL
    assert dotp(plan, None, BH, batch, C, batch, terms) == EINVAL
    assert dotp(plan, A, None, batch, C, batch, terms) == EINVAL
    assert dotp(plan, A, BH, batch, None, batch, terms) == EINVAL
    assert dec(plan, None, D, batch, terms) == EINVAL and dec(plan, A, None, batch, terms) == EINVAL
    for call in (lambda t, w_, f: dotp(plan, A, BH, batch, C, batch, t, w_, f), lambda t, w_, f: dec(plan, A, D, batch, t, w_, f)):
        assert call(0, w, 0) == EINVAL                                              # terms == 0
        assert call(terms, 0, 0) == EINVAL                                          # base_log == 0
        assert call(terms, k, 0) == EINVAL and call(1, 64, 0) == EINVAL             # 2^base_log >= q
        assert call(terms, k - 1, 0) == OK                                          # 2^(k-1) < q, one shift of k - 1
        assert call(4, 22, 0) == EINVAL and call(65, 1, 0) == EINVAL                # (terms - 1) * base_log = 66, 64
        assert call(2, 30, 2) == EINVAL and call(2, 30, 0x80000001) == EINVAL       # an unknown flag bit
    assert dotp(plan, A, BH, 2, C, batch, terms) == EINVAL                          # neither 1 nor batch
    assert dotp(plan, A, BH, batch, A, batch, terms) == EINVAL                      # c is a
    assert dotp(plan, A, BH, batch, BH, batch, terms) == EINVAL                     # c is bhat
    assert dec(plan, A, A, batch, terms) == EINVAL                                  # digits is a
    # c's first row is the last of a's batch rows / the last row of the shared set
    assert dotp(plan, A, BH, batch, A + (batch - 1) * row_bytes, batch, terms) == EINVAL
    assert dotp(plan, A, BH, 1, BH + (terms - 1) * row_bytes, batch, terms) == EINVAL
    # c's last row is the first row of a / of the shared set; the digits' last row is the first row of a
    assert dotp(plan, A, BH, batch, A - (batch - 1) * row_bytes, batch, terms) == EINVAL
    assert dotp(plan, A, BH, 1, BH - (batch - 1) * row_bytes, batch, terms) == EINVAL
    assert dec(plan, A, A - (batch * terms - 1) * row_bytes, batch, terms) == EINVAL
    assert dec(plan, A, A + (batch - 1) * row_bytes, batch, terms) == EINVAL
    # just past the shared set is fine for the overlap check of a shared launch: row `terms` of bhat is not part of it
    assert dotp(plan, A, BH, 1, BH + terms * row_bytes, 1, terms) == OK
    # batch * terms = 2^31: refused before anything is launched (dummy non-NULL pointers)
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_terms, w_ in ((2 ** 31, 1, 30), (2 ** 30, 2, 30), (2 ** 26, 32, 2), (2 ** 25, 64, 1)):
        assert dotp(plan, dummy, dummy, 1, dummy, big_batch, big_terms, w_) == EINVAL, (big_batch, big_terms)
        assert dec(plan, dummy, dummy, big_batch, big_terms, w_) == EINVAL, (big_batch, big_terms)
    assert dotp(plan, None, None, 1, None, 0, 3, 20) == OK                          # batch 0 launches nothing
    assert dec(plan, None, None, 0, 3, 20) == OK
    torch.cuda.synchronize()
    assert torch.equal(c, last)
    assert torch.equal(d, plan.gadget_decompose(a, terms, k - 1))

    # plans without the fused kernels: a general plan, an omega-only plan and n = 16.  The fused call is unsupported there;
    # the decomposition works on every plan.
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    rng = np.random.default_rng(5)
    for other in others:
        assert not other.has_fused
        x = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty_like(x); z = torch.empty_like(x[:2])
        assert dotp(other, x.data_ptr(), y.data_ptr(), 1, z.data_ptr(), 2, 2) == eng.TN_EUNSUPPORTED
        words = rng.integers(0, 2 ** 64 - 1, (3, other.n), dtype=np.uint64, endpoint=True)
        words[0, :3] = (q - 1, q, 2 ** 64 - 1)
        for terms_, w_ in gadget_pairs(q):
            for balanced in MODES:
                got = other.gadget_decompose(words, terms_, w_, balanced)
                assert np.array_equal(got.astype(np.uint64), decompose_rows(words, q, w_, terms_, balanced)), (terms_, w_, balanced)

    # the Python side: a prepared operand is tied to the plan that made it and comes from Plan.prepare
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_gadget_dot_prepared(a, prepared, terms, w)
    with pytest.raises(TypeError):
        plan.poly_gadget_dot_prepared(a, b, terms, w)
    with pytest.raises(ValueError):
        plan.poly_gadget_dot_prepared(a, plan.prepare(b[:3]), terms, w)     # 3 rows: neither terms nor batch * terms
    for bad_terms in (0, -1):
        with pytest.raises(ValueError):
            plan.gadget_decompose(a, bad_terms, w)
        with pytest.raises(ValueError):
            plan.poly_gadget_dot_prepared(a, prepared, bad_terms, w)
