"""GPU tests of the transform-domain entry points (tn_unprepare_dev and tn_poly_dot_hat_dev through Plan.unprepare and
Plan.poly_dot_hat): exact equality with the device's own prepared dot product and fused products, with the oracle and, word
for word, with the CPU stepping, prepared outputs included."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_dot_emu import sum_mod, term_rows
from test_gpu_dot import device_sum
from test_hat_emu import EmuHat
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def hat():
    return EmuHat()


def add_mod(plan, x, y):
    """Word-wise sum mod q of canonical device words: below 2q < 2^63 / 2^32; a sum from 2^31 on shows as negative in a 32-bit
    lane (q > 2^30), is above q, and - q wraps it back."""
    import torch
    s = x + y
    return torch.where((s < 0) | (s >= plan.q), s - plan.q, s)


def rows_of(eng, plan, prepared, first, count):
    """Rows [first, first + count) of a prepared operand, as a prepared operand."""
    return eng.PreparedOperand(plan, prepared.tensor[first:first + count], count)


def host(plan, t):
    return plan.to_host(t).astype(np.uint64)


def check_parity(eng, plan, hat, oracle, n, q, psi, a, b, canonical):
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)               # (the shared rows are read-only; torch wants writable memory to wrap)
    # unprepare is the inverse of prepare, both ways, and equals the stepping
    pa = plan.prepare(a)
    back = plan.unprepare(pa)
    assert back.shape == (5, n)
    assert np.array_equal(host(plan, back), a % np.uint64(q))
    assert torch.equal(plan.prepare(back).tensor, pa.tensor)
    ahat_all = host(plan, pa.tensor)
    assert np.array_equal(host(plan, back), hat.unprepare(n, q, psi, ahat_all, canonical))
    # additivity on the device: prepare(a) + prepare(b) == prepare(a + b), and it unprepares to a + b
    pb = plan.prepare(b)
    word_sum = add_mod(plan, pa.tensor, pb.tensor)
    poly_sum = (a % np.uint64(q) + b % np.uint64(q)) % np.uint64(q)
    assert torch.equal(word_sum, plan.prepare(poly_sum).tensor)
    assert np.array_equal(host(plan, plan.unprepare(eng.PreparedOperand(plan, word_sum, 5))), poly_sum)
    batch = 5
    for terms in (2, 3):
        idx = term_rows(batch, terms)
        flat = idx.ravel()
        a3 = a[idx]                               # (batch, terms, n)
        pa = plan.prepare(a[flat])
        ahat = host(plan, pa.tensor)
        for shared in (False, True):
            bidx = np.tile(np.arange(terms), batch) if shared else flat
            pb = plan.prepare(b[:terms] if shared else b[flat])
            bhat = host(plan, pb.tensor)
            dc = plan.poly_dot_hat(pa, pb, terms)
            assert dc.shape == (batch, n)
            c = host(plan, dc)
            # the device's own prepared dot product and summed fused products
            assert torch.equal(dc, plan.poly_dot_prepared(plan.to_device(a[flat]).reshape(batch, terms, n), pb)), (terms, shared)
            da, db = plan.to_device(a[flat]).reshape(batch, terms, n), plan.to_device(b[bidx]).reshape(batch, terms, n)
            assert torch.equal(dc, device_sum(plan, da, db)), (terms, shared)
            # the oracle
            ref = sum_mod(oracle.poly_mult(a[flat], b[bidx], q, psi).reshape(batch, terms, n), q)
            assert np.array_equal(c, ref), (terms, shared)
            # the stepping, word for word
            assert np.array_equal(c, hat.poly_dot_hat(n, q, psi, ahat, bhat, terms, canonical)), (terms, shared)
            kept = plan.poly_dot_hat(pa, pb, terms, keep_prepared=True)
            assert isinstance(kept, eng.PreparedOperand) and kept.rows == batch and kept.plan is plan
            assert np.array_equal(host(plan, kept.tensor), hat.poly_dot_hat(n, q, psi, ahat, bhat, terms, canonical, keep_prepared=True)), (terms, shared)
            assert torch.equal(kept.tensor, plan.prepare(dc).tensor), (terms, shared)
            assert torch.equal(plan.unprepare(kept), dc), (terms, shared)
    # terms = 1 is the product of two prepared rows
    pa, pb = plan.prepare(a), plan.prepare(b)
    assert torch.equal(plan.poly_dot_hat(pa, pb), plan.poly_mult(plan.to_device(a), plan.to_device(b), variant="fused"))
    one = plan.prepare(b[:1])
    assert torch.equal(plan.poly_dot_hat(pa, one), plan.poly_mult_prepared(plan.to_device(a), one))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_hat_equals_prepared_dot_fused_products_oracle_and_stepping(eng, hat, oracle, case):
    n, q, psi, a, b = _case_data(case)
    check_parity(eng, eng.get_plan(n, q, psi), hat, oracle, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_hat_on_a_canonical_policy_plan(eng, hat, oracle, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(eng, plan, hat, oracle, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_small_and_large_batches(eng, tag):
    """terms = 2 at batch 1, 7 and a batch above any grid of resident workgroups (16 workgroups of two waves, 4 of eight waves
    per CU at the most): two launches agree with each other and with the prepared dot product on the un-prepared a, prepared
    outputs unprepare to the same rows, and every input is left unchanged."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (16 if n == 1024 else 4) * cus + 5
    terms = 2
    shared = plan.prepare(plan.fill_lcg(terms, 77, 2))
    per_set = plan.prepare(plan.fill_lcg(big * terms, 2, 2))
    a_all = plan.fill_lcg(big * terms, 1, 2)
    pa_all = plan.prepare(a_all)
    before = shared.tensor.clone(), per_set.tensor.clone(), pa_all.tensor.clone()
    for batch in (1, 7, big):
        a3 = a_all[:batch * terms].reshape(batch, terms, n)
        pa = rows_of(eng, plan, pa_all, 0, batch * terms)
        for pb in (shared, rows_of(eng, plan, per_set, 0, batch * terms)):
            c1 = plan.poly_dot_hat(pa, pb, terms)
            c2 = plan.poly_dot_hat(pa, pb, terms)
            assert torch.equal(c1, plan.poly_dot_prepared(a3, pb)), (tag, batch)
            assert torch.equal(c1, c2), (tag, batch)
            kept = plan.poly_dot_hat(pa, pb, terms, keep_prepared=True)
            assert torch.equal(plan.unprepare(kept), c1), (tag, batch)
            assert torch.equal(kept.tensor, plan.prepare(c1).tensor), (tag, batch)
        assert torch.equal(plan.unprepare(pa), a_all[:batch * terms]), (tag, batch)          # fill_lcg words are canonical
    assert torch.equal(shared.tensor, before[0]) and torch.equal(per_set.tensor, before[1]) and torch.equal(pa_all.tensor, before[2])


def test_dynamic_row_hand_out(eng, emu, oracle):
    """Enough rows at n = 4096 / 60-bit for plan_rows to hand rows out through the device counter: for each kernel the smallest
    batch that launch_plan.h's plan_rows calls dynamic for its row size (terms * n * 8 bytes for the dot product at terms = 2,
    n * 8 bytes for unprepare) when 4 workgroups per CU are resident, which is above what any fused kernel of this size reaches."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms = 2
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count

    def smallest_dynamic(row_bytes):
        return smallest_dynamic_batch(row_bytes, resident)

    rows = smallest_dynamic(terms * n * plan.elem_bytes)
    a = plan.fill_lcg(rows * terms, 1, 2); b = plan.fill_lcg(rows * terms, 2, 2)
    a3 = a.reshape(rows, terms, n)
    pa, pb = plan.prepare(a), plan.prepare(b)
    c = plan.poly_dot_hat(pa, pb, terms)
    assert torch.equal(c, plan.poly_dot_prepared(a3, pb))
    shared = rows_of(eng, plan, pb, 0, terms)
    c_shared = plan.poly_dot_hat(pa, shared, terms)
    assert torch.equal(c_shared, plan.poly_dot_prepared(a3, shared))
    for ref, pb_ in ((c, pb), (c_shared, shared)):
        kept = plan.poly_dot_hat(pa, pb_, terms, keep_prepared=True)
        assert torch.equal(kept.tensor, plan.prepare(ref).tensor)
    idx = [0, 1, 511, 512, 1777, 3071, 3072, rows - 1]
    sel = torch.tensor(idx, device=a.device)
    ha = plan.to_host(a3[sel].reshape(-1, n)); hb = plan.to_host(b.reshape(rows, terms, n)[sel].reshape(-1, n))
    ref = sum_mod(oracle.poly_mult(ha, hb, q, psi).reshape(len(idx), terms, n), q)
    assert np.array_equal(host(plan, c[sel]), ref)
    # unprepare: its own row size
    urows = smallest_dynamic(n * plan.elem_bytes)
    assert urows <= rows * terms
    assert torch.equal(plan.unprepare(rows_of(eng, plan, pa, 0, urows)), a[:urows])             # fill_lcg words are canonical


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
        pa, pb = plan.prepare(a, stream=side), plan.prepare(b, stream=side)
        c = plan.poly_dot_hat(pa, pb, terms, stream=side)
        kept = plan.poly_dot_hat(pa, rows_of(eng, plan, pb, 0, terms), terms, keep_prepared=True)      # stream=None: torch's current stream, `side` here
        c_shared = plan.unprepare(kept, stream=side)
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c_shared, ref_shared)


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, terms = 5, 2
    a = plan.fill_lcg(batch * terms, 1, 2); b = plan.fill_lcg(batch * terms, 2, 2)
    pa, pb = plan.prepare(a), plan.prepare(b)
    c = torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device)
    x = torch.empty((batch * terms, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    AH, BH, C, X = pa.tensor.data_ptr(), pb.tensor.data_ptr(), c.data_ptr(), x.data_ptr()
    row_bytes = n * plan.elem_bytes

    def doth(p, ah, bh, sets, c_, batch_, terms_, keep=0):
        return lib.tn_poly_dot_hat_dev(p._h, ah, bh, sets, c_, batch_, terms_, keep, stream)

    assert doth(plan, AH, BH, batch, C, batch, terms) == eng.TN_OK
    assert lib.tn_poly_dot_hat_dev(None, AH, BH, batch, C, batch, terms, 0, stream) == eng.TN_EINVAL               # NULL plan
    assert doth(plan, None, BH, batch, C, batch, terms) == eng.TN_EINVAL
    assert doth(plan, AH, None, batch, C, batch, terms) == eng.TN_EINVAL
    assert doth(plan, AH, BH, batch, None, batch, terms) == eng.TN_EINVAL
    assert doth(plan, AH, BH, batch, C, batch, 0) == eng.TN_EINVAL                                                 # terms == 0
    assert doth(plan, AH, BH, 2, C, batch, terms) == eng.TN_EINVAL                                                 # neither 1 nor batch
    for keep in (2, -1):
        assert doth(plan, AH, BH, batch, C, batch, terms, keep) == eng.TN_EINVAL                                   # out_prepared not in {0, 1}
    for keep in (0, 1):
        assert doth(plan, AH, BH, batch, AH, batch, terms, keep) == eng.TN_EINVAL                                  # out is ahat
        assert doth(plan, AH, BH, batch, BH, batch, terms, keep) == eng.TN_EINVAL                                  # out is bhat
        # out's first row is the last of ahat's batch * terms rows / the last row of the shared set
        assert doth(plan, AH, BH, batch, AH + (batch * terms - 1) * row_bytes, batch, terms, keep) == eng.TN_EINVAL
        assert doth(plan, AH, BH, 1, BH + (terms - 1) * row_bytes, batch, terms, keep) == eng.TN_EINVAL
        # out's last row is the first row of ahat / of the shared set
        assert doth(plan, AH, BH, batch, AH - (batch - 1) * row_bytes, batch, terms, keep) == eng.TN_EINVAL
        assert doth(plan, AH, BH, 1, BH - (batch - 1) * row_bytes, batch, terms, keep) == eng.TN_EINVAL
    # just past the shared set is fine for the overlap check of a shared launch: row `terms` of bhat is not part of it
    spare = pb.tensor.clone()
    assert doth(plan, AH, spare.data_ptr(), 1, spare.data_ptr() + terms * row_bytes, 1, terms) == eng.TN_OK
    # batch * terms = 2^31: refused before anything is launched (dummy non-NULL pointers)
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_terms in ((2 ** 31, 1), (2 ** 30, 2), (1, 2 ** 31), (2 ** 16, 2 ** 15), (3, 2 ** 63)):
        assert doth(plan, dummy, dummy, 1, dummy, big_batch, big_terms) == eng.TN_EINVAL, (big_batch, big_terms)
    assert doth(plan, None, None, 1, None, 0, 3) == eng.TN_OK                                                      # batch 0 launches nothing

    def unprep(p, xh, x_, rows_):
        return lib.tn_unprepare_dev(p._h, xh, x_, rows_, stream)

    assert unprep(plan, AH, X, batch * terms) == eng.TN_OK
    assert lib.tn_unprepare_dev(None, AH, X, batch * terms, stream) == eng.TN_EINVAL
    assert unprep(plan, None, X, batch * terms) == eng.TN_EINVAL
    assert unprep(plan, AH, None, batch * terms) == eng.TN_EINVAL
    assert unprep(plan, AH, AH, batch * terms) == eng.TN_EINVAL                                                    # x is xhat
    assert unprep(plan, AH, AH + (batch * terms - 1) * row_bytes, batch * terms) == eng.TN_EINVAL
    assert unprep(plan, AH, AH - (batch * terms - 1) * row_bytes, batch * terms) == eng.TN_EINVAL
    assert unprep(plan, dummy, dummy, 2 ** 31) == eng.TN_EINVAL
    assert unprep(plan, None, None, 0) == eng.TN_OK                                                                # rows 0 launches nothing
    torch.cuda.synchronize()
    assert torch.equal(c, plan.poly_dot_prepared(a.reshape(batch, terms, n), pb))
    assert torch.equal(x, a)                                                                                       # fill_lcg words are canonical
    assert torch.equal(pa.tensor, plan.prepare(a).tensor) and torch.equal(pb.tensor, plan.prepare(b).tensor)

    # plans without the fused kernels: a general plan, an omega-only plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    for other in others:
        assert not other.has_fused
        u = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); v = torch.empty_like(u); w = torch.empty_like(u[:2])
        for keep in (0, 1):
            assert doth(other, u.data_ptr(), v.data_ptr(), 2, w.data_ptr(), 2, 2, keep) == eng.TN_EUNSUPPORTED
        assert unprep(other, u.data_ptr(), v.data_ptr(), 4) == eng.TN_EUNSUPPORTED

    # the Python side: prepared operands are tied to the plan that made them and come from Plan.prepare / keep_prepared
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_dot_hat(pa, cplan.prepare(b), terms)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_dot_hat(cplan.prepare(a), pb, terms)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.unprepare(pa)
    with pytest.raises(TypeError):
        plan.poly_dot_hat(a, pb, terms)
    with pytest.raises(TypeError):
        plan.poly_dot_hat(pa, b, terms)
    with pytest.raises(TypeError):
        plan.unprepare(a)
    with pytest.raises(ValueError):
        plan.poly_dot_hat(pa, pb, 3)                                      # 10 rows are no multiple of 3 terms
    with pytest.raises(ValueError):
        plan.poly_dot_hat(pa, rows_of(eng, plan, pb, 0, 3), terms)        # 3 rows: neither terms nor batch * terms


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_matrix_times_vector_equals_prepared_dot_calls(eng, tag):
    """c[i] = sum_j A[i][j] * s[j] for a fixed 3 x 3 matrix over 4 vectors: the vectors' 3 rows prepared once plus 3 dot products
    of prepared rows against the matrix rows as shared sets, against 3 prepared dot products on the un-prepared vectors."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    k = l = 3
    vectors = 4
    mat = plan.prepare(plan.fill_lcg(k * l, 11, 2))                        # A[i][j] at row i * l + j
    s = plan.fill_lcg(vectors * l, 12, 2)                                  # s[v][j] at row v * l + j
    shat = plan.prepare(s)
    for i in range(k):
        row_i = rows_of(eng, plan, mat, i * l, l)
        new = plan.poly_dot_hat(shat, row_i, l)
        old = plan.poly_dot_prepared(s.reshape(vectors, l, n), row_i)
        assert new.shape == (vectors, n) and torch.equal(new, old), (tag, i)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_accumulate_across_launches(eng, tag):
    """Two results kept prepared, added mod q on the device and unprepared once: the sum of the two coefficient results."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    batch, terms = 6, 2
    pa0, pa1 = plan.prepare(plan.fill_lcg(batch * terms, 21, 2)), plan.prepare(plan.fill_lcg(batch * terms, 22, 2))
    pb0, pb1 = plan.prepare(plan.fill_lcg(batch * terms, 23, 2)), plan.prepare(plan.fill_lcg(terms, 24, 2))
    c0, c1 = plan.poly_dot_hat(pa0, pb0, terms), plan.poly_dot_hat(pa1, pb1, terms)
    h0 = plan.poly_dot_hat(pa0, pb0, terms, keep_prepared=True)
    h1 = plan.poly_dot_hat(pa1, pb1, terms, keep_prepared=True)
    total = eng.PreparedOperand(plan, add_mod(plan, h0.tensor, h1.tensor), batch)
    assert torch.equal(plan.unprepare(total), add_mod(plan, c0, c1)), tag
    # ... and a kept result is an operand of the next product: (a0 . b0) * b1[0] against the product of the coefficients
    nxt = plan.poly_dot_hat(h0, rows_of(eng, plan, pb1, 0, 1))
    assert torch.equal(nxt, plan.poly_mult_prepared(c0, rows_of(eng, plan, pb1, 0, 1))), tag
