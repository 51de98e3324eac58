"""GPU tests of tn_poly_external_product_prepared_dev (Plan.poly_external_product_prepared): the external product RGSW x RLWE from
one launch, bit for bit against route B on the device (tn_gadget_decompose_dev on the batch * ins rows, then
tn_poly_dot_prepared_dev with ins * terms terms per component) and against the CPU stepping of the kernel (tests/emu/emu_extprod.cpp)."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_extprod_emu import INS, EmuExtprod, ext_rows, input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def extprod():
    return EmuExtprod()


def component(eng, plan, prepared, batch, outs, ins, terms, o):
    """Component o of an external-product operand ([sets][outs][ins][terms] rows) as an operand of the dot product with
    ins * terms terms."""
    n, it = plan.n, ins * terms
    if prepared.rows == outs * it:
        return eng.PreparedOperand(plan, prepared.tensor[o * it:(o + 1) * it], it)
    rows = prepared.tensor.reshape(batch, outs, it, n)[:, o].contiguous().reshape(batch * it, n)
    return eng.PreparedOperand(plan, rows, batch * it)


def route_b(eng, plan, a, prepared, outs, terms, w, balanced):
    """The contract: gadget_decompose on the (batch * ins, n) view of a, then poly_dot_prepared per component -> (batch, outs, n)."""
    import torch
    batch, ins, n = a.shape
    digits = plan.gadget_decompose(a.reshape(batch * ins, n), terms, w, balanced).reshape(batch, ins * terms, n)
    return torch.stack([plan.poly_dot_prepared(digits, component(eng, plan, prepared, batch, outs, ins, terms, o)) for o in range(outs)], dim=1)


def check_parity(eng, plan, extprod, n, q, psi, a, b, canonical, ins_list=INS, pairs=None):
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)
    batch = 5
    first = 0
    for ins in ins_list:
        for terms, w in pairs or gadget_pairs(q):
            ha = a[input_rows(batch, ins, first)]                        # (batch, ins, n)
            first += 1
            da = plan.to_device(ha.reshape(batch * ins, n)).reshape(batch, ins, n)
            for shared in (True, False):
                idx = ext_rows(batch, ins, terms)
                prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
                assert prepared.rows == (2 * ins * terms if shared else batch * 2 * ins * terms)
                bhat = plan.to_host(prepared.tensor).astype(np.uint64)
                for balanced in MODES:
                    where = (ins, terms, w, shared, balanced)
                    c = plan.poly_external_product_prepared(da, prepared, 2, terms, w, balanced)
                    assert c.shape == (batch, 2, n)
                    assert torch.equal(c, route_b(eng, plan, da, prepared, 2, terms, w, balanced)), where
                    hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(batch, 2, n)
                    assert np.array_equal(hc, extprod.external_product(n, q, psi, ha, bhat, terms, w, balanced, canonical)), where
    return ha, da


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_external_product_equals_route_b_and_the_stepping(eng, extprod, case):
    n, q, psi, a, b = _case_data(case)
    plan = eng.get_plan(n, q, psi)
    check_parity(eng, plan, extprod, n, q, psi, a, b, False)
    # host arrays in, host arrays out; one ciphertext: (ins, n) in, (outs, n) out
    terms, w = gadget_pairs(q)[1]
    ha = np.array(a)[input_rows(5, 2)]
    da = plan.to_device(ha.reshape(10, n)).reshape(5, 2, n)
    prepared = plan.prepare(np.array(b)[ext_rows(1, 2, terms)[0].ravel()])
    ref = plan.to_host(route_b(eng, plan, da, prepared, 2, terms, w, True).reshape(-1, n)).reshape(5, 2, n)
    hc = plan.poly_external_product_prepared(ha, prepared, 2, terms, w, True)
    assert isinstance(hc, np.ndarray) and hc.shape == (5, 2, n) and np.array_equal(hc, ref)
    one = plan.poly_external_product_prepared(ha[2], prepared, 2, terms, w, True)
    assert isinstance(one, np.ndarray) and one.shape == (2, n) and np.array_equal(one, ref[2])
    one = plan.poly_external_product_prepared(da[2], prepared, 2, terms, w, True)
    assert one.shape == (2, n) and np.array_equal(plan.to_host(one), ref[2])


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_external_product_on_a_canonical_policy_plan(eng, extprod, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(eng, plan, extprod, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_one_input_is_the_multidot_call(eng, tag):
    """ins = 1 with one and with two components: the multidot call's kernels, its results."""
    import torch
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi)
    da = plan.to_device(np.array(a))
    terms, w = gadget_pairs(q)[1]
    for outs in (1, 2):
        for rows in (outs * terms, 5 * outs * terms):
            prepared = plan.prepare(np.array(b)[np.arange(rows) % 5])
            for balanced in MODES:
                c = plan.poly_external_product_prepared(da.reshape(5, 1, n), prepared, outs, terms, w, balanced)
                assert c.shape == (5, outs, n)
                assert torch.equal(c, plan.poly_gadget_multidot_prepared(da, prepared, outs, terms, w, balanced)), (outs, rows, balanced)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_small_and_large_batches(eng, tag):
    """ins = terms = 2 at batch 1, 7 and a batch above any grid of resident workgroups: two launches agree with each other and
    with route B, and leave the prepared rows and a alone."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (16 if n == 1024 else 4) * cus + 5
    ins = 2
    terms, w = gadget_pairs(q)[0]
    shared = plan.prepare(plan.fill_lcg(2 * ins * terms, 77, 2))
    per_set = plan.prepare(plan.fill_lcg(big * 2 * ins * terms, 2, 2))
    a_all = plan.fill_lcg(big * ins, 1, 2).reshape(big, ins, n)
    before = shared.tensor.clone(), per_set.tensor.clone(), a_all.clone()
    for batch in (1, 7, big):
        a = a_all[:batch]
        for prepared in (shared, eng.PreparedOperand(plan, per_set.tensor[:batch * 2 * ins * terms], batch * 2 * ins * terms)):
            for balanced in MODES:
                c1 = plan.poly_external_product_prepared(a, prepared, 2, terms, w, balanced)
                c2 = plan.poly_external_product_prepared(a, prepared, 2, terms, w, balanced)
                assert torch.equal(c1, route_b(eng, plan, a, prepared, 2, terms, w, balanced)), (tag, batch, balanced)
                assert torch.equal(c1, c2), (tag, batch, balanced)
    assert torch.equal(shared.tensor, before[0]) and torch.equal(per_set.tensor, before[1]) and torch.equal(a_all, before[2])


def test_dynamic_row_hand_out(eng, extprod):
    """Enough output rows at n = 4096 / 60-bit, ins = terms = 2 for plan_rows to hand rows out through the device counter: the
    launcher plans an output row with dot_row_bytes(n * 8, ins * terms), here ins * terms + 2 transforms between two atomics."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    ins, terms, w = 2, 2, 30
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = smallest_dynamic_batch(ins * terms * n * plan.elem_bytes, resident)
    a = plan.fill_lcg(rows * ins, 1, 2).reshape(rows, ins, n); b = plan.fill_lcg(rows * 2 * ins * terms, 2, 2)
    per_set, shared = plan.prepare(b), plan.prepare(b[:2 * ins * terms])
    c = plan.poly_external_product_prepared(a, per_set, 2, terms, w, True)
    assert torch.equal(c, route_b(eng, plan, a, per_set, 2, terms, w, True))
    c_shared = plan.poly_external_product_prepared(a, shared, 2, terms, w, True)
    assert torch.equal(c_shared, route_b(eng, plan, a, shared, 2, terms, w, True))
    # a few rows, among them the first and last of the launch and of chunks in between, against the CPU stepping
    idx = sorted({0, 1, rows // 6 - 1, rows // 6, 1777 % rows, rows // 2 - 1, rows // 2, rows - 1})
    sel = torch.tensor(idx, device=a.device)
    ha = plan.to_host(a[sel].reshape(-1, n)).astype(np.uint64).reshape(len(idx), ins, n)
    hb = plan.to_host(per_set.tensor.reshape(rows, 2 * ins * terms, n)[sel].reshape(-1, n)).astype(np.uint64)
    got = plan.to_host(c[sel].reshape(-1, n)).astype(np.uint64).reshape(len(idx), 2, n)
    assert np.array_equal(got, extprod.external_product(n, q, psi, ha, hb, terms, w, True))


def test_launch_on_a_side_stream(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    ins, terms, w = 3, 3, 20
    a = plan.fill_lcg(9 * ins, 5, 2).reshape(9, ins, n); b = plan.fill_lcg(9 * 2 * ins * terms, 6, 2)
    per_set, shared = plan.prepare(b), plan.prepare(b[:2 * ins * terms])
    ref = route_b(eng, plan, a, per_set, 2, terms, w, True)
    ref_shared = route_b(eng, plan, a, shared, 2, terms, w, False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = plan.poly_external_product_prepared(a, per_set, 2, terms, w, True, stream=side)
        c_shared = plan.poly_external_product_prepared(a, shared, 2, terms, w)     # stream=None: torch's current stream, `side` here
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c_shared, ref_shared)


def test_capture_into_a_graph(eng):
    """One launch captured into a graph (one kernel node, no parallel branches) and replayed twice onto a zeroed output: a
    captured launch runs the fixed row stride."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    ins, terms, w = 2, 2, 30
    rows = 1500
    a = plan.fill_lcg(rows * ins, 3, 2).reshape(rows, ins, n); b = plan.fill_lcg(rows * 2 * ins * terms, 4, 2)
    prepared = plan.prepare(b)
    ref = route_b(eng, plan, a, prepared, 2, terms, w, True)
    s1 = torch.cuda.Stream(); c = torch.zeros_like(ref)
    torch.cuda.synchronize()          # the inputs, the reference and the zero fill ran on the default stream: s1 starts behind them
    with torch.cuda.stream(s1):
        plan.poly_external_product_prepared(a, prepared, 2, terms, w, True, out=c, stream=s1)     # warm-up outside the capture
    s1.synchronize()
    assert torch.equal(c, ref)
    g = torch.cuda.CUDAGraph(); c.zero_(); torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s1):
        plan.poly_external_product_prepared(a, prepared, 2, terms, w, True, out=c, stream=s1)
    for rep in range(2):
        c.zero_(); torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(c, ref), rep


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    k = q.bit_length()
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, ins, outs, terms, w = 5, 2, 2, 2, 30
    a = plan.fill_lcg(batch * ins, 1, 2).reshape(batch, ins, n); b = plan.fill_lcg(batch * outs * ins * terms, 2, 2)
    prepared = plan.prepare(b)
    c = torch.empty((batch, outs, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, BH, C = a.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr()
    row_bytes = n * plan.elem_bytes
    OK, EINVAL, EUNSUPPORTED = eng.TN_OK, eng.TN_EINVAL, eng.TN_EUNSUPPORTED
    fn = lib.tn_poly_external_product_prepared_dev

    def call(p, a_, bh, sets, c_, batch_, ins_, outs_, terms_, w_=w, flags=0):
        return fn(p._h, a_, bh, sets, c_, batch_, ins_, outs_, terms_, w_, flags, stream)

    last = route_b(eng, plan, a, prepared, outs, terms, k - 1, False)       # what the last accepted launch into c below computes
    assert call(plan, A, BH, batch, C, batch, ins, outs, terms) == OK
    assert call(plan, A, BH, batch, C, batch, ins, outs, terms, w, eng.GADGET_BALANCED) == OK
    assert fn(None, A, BH, batch, C, batch, ins, outs, terms, w, 0, stream) == EINVAL                  # NULL plan
    assert call(plan, None, BH, batch, C, batch, ins, outs, terms) == EINVAL
    assert call(plan, A, None, batch, C, batch, ins, outs, terms) == EINVAL
    assert call(plan, A, BH, batch, None, batch, ins, outs, terms) == EINVAL
    assert call(plan, A, BH, batch, C, batch, 0, outs, terms) == EINVAL                       # ins == 0
    assert b"ins must be at least 1" in lib.tn_last_error()
    assert call(plan, A, BH, batch, C, batch, ins, 0, terms) == EINVAL                        # outs == 0
    assert call(plan, A, BH, batch, C, batch, ins, 3, terms) == EUNSUPPORTED                  # more than two components
    assert b"more than 2" in lib.tn_last_error()
    assert call(plan, A, BH, batch, C, batch, ins, 1, terms) == EUNSUPPORTED                  # two inputs into one component
    assert b"into 1 output component" in lib.tn_last_error()
    assert call(plan, A, BH, batch, C, batch, 3, 1, terms) == EUNSUPPORTED
    assert call(plan, A, BH, batch, C, batch, ins, outs, 0) == EINVAL                         # terms == 0
    assert call(plan, A, BH, batch, C, batch, ins, outs, terms, 0) == EINVAL                  # base_log == 0
    assert call(plan, A, BH, batch, C, batch, ins, outs, terms, k) == EINVAL                  # 2^base_log >= q
    assert call(plan, A, BH, batch, C, batch, ins, outs, 4, 22) == EINVAL                     # (terms - 1) * base_log = 66
    assert call(plan, A, BH, batch, C, batch, ins, outs, terms, w, 2) == EINVAL               # an unknown flag bit
    assert call(plan, A, BH, 2, C, batch, ins, outs, terms) == EINVAL                         # neither 1 nor batch
    assert call(plan, A, BH, batch, A, batch, ins, outs, terms) == EINVAL                     # c is a
    assert call(plan, A, BH, batch, BH, batch, ins, outs, terms) == EINVAL                    # c is bhat
    assert call(plan, A, BH, batch, A + (batch * ins - 1) * row_bytes, batch, ins, outs, terms) == EINVAL      # c's first row is a's last
    assert call(plan, A, BH, batch, A - (batch * outs - 1) * row_bytes, batch, ins, outs, terms) == EINVAL     # c's last row is a's first
    assert call(plan, A, BH, 1, BH + (outs * ins * terms - 1) * row_bytes, batch, ins, outs, terms) == EINVAL  # ... the shared set's last
    assert call(plan, A, BH, 1, BH - (batch * outs - 1) * row_bytes, batch, ins, outs, terms) == EINVAL        # ... the shared set's first
    assert call(plan, A, BH, batch, C, batch, ins, outs, terms, k - 1) == OK                  # 2^(k-1) < q, one shift of k - 1
    # just past the shared set is fine for the overlap check of a shared launch: row outs * ins * terms of bhat is not part of it
    # (this launch writes into rows of bhat that no later launch into c reads)
    assert call(plan, A, BH, 1, BH + outs * ins * terms * row_bytes, 1, ins, outs, terms) == OK
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_ins, big_terms, w_ in ((2 ** 29, 2, 1, 30), (2 ** 28, 2, 2, 30), (2 ** 24, 2, 32, 2), (2, 2 ** 62, 1, 30), (2 ** 63, 2, 1, 30)):
        assert call(plan, dummy, dummy, 1, dummy, big_batch, big_ins, outs, big_terms, w_) == EINVAL, (big_batch, big_ins, big_terms)
        assert b"batch * outs * ins * terms too large" in lib.tn_last_error()
    assert call(plan, None, None, 1, None, 0, ins, outs, 3, 20) == OK                         # batch 0 launches nothing
    torch.cuda.synchronize()
    assert torch.equal(c, last)

    # plans without the fused kernels: a general plan, an omega-only plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    for other in others:
        assert not other.has_fused
        x = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty((8, other.n), dtype=other.torch_dtype, device="cuda:0")
        z = torch.empty_like(x)
        assert call(other, x.data_ptr(), y.data_ptr(), 1, z.data_ptr(), 2, 2, 2, 2) == EUNSUPPORTED
        assert b"fused kernels" in lib.tn_last_error()

    # the Python side
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_external_product_prepared(a, prepared, outs, terms, w)
    with pytest.raises(TypeError):
        plan.poly_external_product_prepared(a, b, outs, terms, w)
    with pytest.raises(ValueError):
        plan.poly_external_product_prepared(a, plan.prepare(b[:3]), outs, terms, w)     # 3 rows: neither one set nor batch sets
    with pytest.raises(ValueError):
        plan.poly_external_product_prepared(a.reshape(-1), prepared, outs, terms, w)     # a needs (batch, ins, n) or (ins, n)
    with pytest.raises(ValueError):
        plan.poly_external_product_prepared(a[:, :, :n - 1], prepared, outs, terms, w)
    with pytest.raises(eng.TinyNttError):
        plan.poly_external_product_prepared(a[:, :1], prepared, outs, 2 * terms, w)      # a view that is not contiguous
    with pytest.raises(eng.TinyNttError, match="into 1 output component"):
        plan.poly_external_product_prepared(a, plan.prepare(b[:ins * terms]), 1, terms, w)
    # out is checked like poly_gadget_multidot_prepared's: a host tensor or another word size never reaches the kernel
    with pytest.raises(eng.TinyNttError):
        plan.poly_external_product_prepared(a, prepared, outs, terms, w, out=torch.empty((batch, outs, n), dtype=plan.torch_dtype))
    with pytest.raises(eng.TinyNttError):
        plan.poly_external_product_prepared(a, prepared, outs, terms, w, out=torch.empty((batch, outs, n), dtype=torch.int32, device=a.device))
    with pytest.raises(ValueError):
        plan.poly_external_product_prepared(a, prepared, outs, terms, w, out=torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            plan.poly_external_product_prepared(a, prepared, outs, bad, w)
        with pytest.raises(ValueError):
            plan.poly_external_product_prepared(a, prepared, bad, terms, w)
    torch.cuda.synchronize()
    assert torch.equal(c, last)
