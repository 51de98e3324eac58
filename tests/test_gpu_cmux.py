"""GPU tests of tn_monomial_mul_dev and tn_poly_cmux_rotate_prepared_dev (Plan.monomial_mul, Plan.poly_cmux_rotate_prepared,
Plan.blind_rotate): one step of a blind rotation from one launch, bit for bit against the explicit route on the device
(tn_monomial_mul_dev with TN_MONOMIAL_MINUS_ONE, tn_poly_external_product_prepared_dev, the addition mod q) and against the CPU
stepping of the kernel (tests/emu/emu_cmux.cpp); the monomial product against the numpy statement of its definition."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_cmux_emu import BATCH, TRIVIAL, EmuCmux, exponents, key_rows, monomial_np, trivial_key
from test_extprod_emu import input_rows
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
def cmux():
    return EmuCmux()


def dev_exps(exps):
    import torch
    return torch.from_numpy(np.ascontiguousarray(exps, dtype=np.uint32).view(np.int32)).to("cuda:0")


def add_mod(plan, a, p):
    """(a mod q + p) mod q word by word for canonical p: a mod q is sigma_1 (tn_automorphism_dev with g = 1: canonicalisation);
    the sum is taken in 64 bits (2q fits neither a signed 32-bit word nor, as a bit pattern, needs to: q < 2^62)."""
    import torch
    n = plan.n
    amod = plan.automorphism(a.reshape(-1, n), 1).reshape(a.shape).to(torch.int64)
    s = amod + p.to(torch.int64)
    return torch.where(s >= plan.q, s - plan.q, s).to(plan.torch_dtype)


def explicit(plan, a, exps, prepared, terms, w, balanced):
    """The contract: monomial_mul(minus_one) on (batch, 2, n), poly_external_product_prepared with ins = outs = 2, the addition."""
    m = plan.monomial_mul(a, exps, minus_one=True)
    return add_mod(plan, a, plan.poly_external_product_prepared(m, prepared, 2, terms, w, balanced))


def check_parity(eng, plan, cmux, n, q, psi, a, b, canonical, pairs=None):
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)
    exps = exponents(n)
    de = dev_exps(exps)
    for first, (terms, w) in enumerate(pairs or gadget_pairs(q)):
        ha = np.ascontiguousarray(a[input_rows(BATCH, 2, first)])            # (7, 2, n)
        da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
            assert prepared.rows == (4 * terms if shared else BATCH * 4 * terms)
            bhat = plan.to_host(prepared.tensor).astype(np.uint64)
            for balanced in MODES:
                where = (terms, w, shared, balanced)
                c = plan.poly_cmux_rotate_prepared(da, de, prepared, terms, w, balanced)
                assert c.shape == (BATCH, 2, n)
                assert torch.equal(c, explicit(plan, da, de, prepared, terms, w, balanced)), where
                hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
                assert np.array_equal(hc, cmux.rotate(n, q, psi, ha, exps, bhat, terms, w, balanced, canonical)), where
    return ha, da


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_rotation_equals_the_explicit_route_and_the_stepping(eng, cmux, case):
    n, q, psi, a, b = _case_data(case)
    plan = eng.get_plan(n, q, psi)
    check_parity(eng, plan, cmux, n, q, psi, a, b, False)
    # host arrays in, host arrays out, host exponents of any size; one ciphertext: (2, n) in, (2, n) out
    terms, w = gadget_pairs(q)[1]
    exps = exponents(n)
    ha = np.array(a)[input_rows(BATCH, 2)]
    da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
    prepared = plan.prepare(np.array(b)[key_rows(1, terms, True)[0].ravel()])
    ref = plan.to_host(explicit(plan, da, dev_exps(exps), prepared, terms, w, True).reshape(-1, n)).reshape(BATCH, 2, n)
    hc = plan.poly_cmux_rotate_prepared(ha, [int(e) + 4 * n for e in exps], prepared, terms, w, True)
    assert isinstance(hc, np.ndarray) and hc.shape == (BATCH, 2, n) and np.array_equal(hc, ref)
    one = plan.poly_cmux_rotate_prepared(ha[2], [int(exps[2])], prepared, terms, w, True)
    assert isinstance(one, np.ndarray) and one.shape == (2, n) and np.array_equal(one, ref[2])
    one = plan.poly_cmux_rotate_prepared(da[2], dev_exps(exps[2:3]), prepared, terms, w, True)
    assert one.shape == (2, n) and np.array_equal(plan.to_host(one), ref[2])


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_rotation_on_a_canonical_policy_plan(eng, cmux, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(eng, plan, cmux, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag", ["P256", "P1024", "P4096_60"])
def test_trivial_rgsw_of_a_bit_selects_the_rotation(eng, tag):
    """A noise-free trivial RGSW of a bit m with unsigned digits that cover q (tests/test_cmux_emu.py): the step returns rot_e(a)
    for m = 1 and a mod q for m = 0, word for word; nothing here passes through the project's decomposition."""
    n, q, psi, a, _ = _case_data(tag)
    plan = eng.get_plan(n, q, psi)
    terms, w = TRIVIAL[q.bit_length()]
    exps = exponents(n)
    ha = np.ascontiguousarray(np.array(a)[input_rows(BATCH, 2)])
    da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
    for m in (0, 1):
        prepared = plan.prepare(trivial_key(n, q, m, terms, w))
        c = plan.poly_cmux_rotate_prepared(da, dev_exps(exps), prepared, terms, w)
        want = monomial_np(ha, exps, q) if m else ha % np.uint64(q)
        assert np.array_equal(plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n), want), (tag, m)


def test_monomial_product_on_every_kind_of_plan(eng):
    """tn_monomial_mul_dev on a fused plan, a general plan, an omega-only plan and n = 16, both lane widths: against the numpy
    statement of the definition for both flags, group 1 and 2, device and host arrays, any words and unreduced exponents."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    n2, q2, psi2 = PARAMS["P1024"]
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    plans = [eng.get_plan(n, q, psi), eng.get_plan(n2, q2, psi2), eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)),
             eng.get_general_plan(n2, q2, psi2), eng.get_plan(16, q, small_psi)]
    rng = np.random.default_rng(5)
    for plan in plans:
        pn, pq = plan.n, plan.q
        exps = np.concatenate([exponents(pn), rng.integers(0, 2 ** 32, 4, dtype=np.uint64).astype(np.uint32)])
        batch = len(exps)
        word = 2 ** (8 * plan.elem_bytes) - 1
        for group in (1, 2):
            ha = rng.integers(0, word, (batch, group, pn), dtype=np.uint64, endpoint=True)
            ha[0, 0, :3] = (0, pq, pq - 1)
            da = plan.to_device(ha.reshape(batch * group, pn)).reshape(batch, group, pn)
            for minus_one in (False, True):
                where = (pn, pq, plan.general, plan.omega_only, group, minus_one)
                want = monomial_np(ha, exps, pq, minus_one)
                out = plan.monomial_mul(da, dev_exps(exps), minus_one)
                assert out.shape == (batch, group, pn)
                assert np.array_equal(plan.to_host(out.reshape(-1, pn)).astype(np.uint64).reshape(want.shape), want), where
                host = plan.monomial_mul(ha.astype(plan.dtype), [int(e) for e in exps], minus_one)
                assert isinstance(host, np.ndarray) and np.array_equal(host.astype(np.uint64), want), where
        # (batch, n): one row per exponent
        flat = plan.monomial_mul(da[:, 0].contiguous(), dev_exps(exps))
        assert flat.shape == (batch, pn) and np.array_equal(plan.to_host(flat).astype(np.uint64), monomial_np(ha[:, :1], exps, pq)[:, 0])
        assert torch.equal(da, plan.to_device(ha.reshape(batch * group, pn)).reshape(batch, group, pn))      # the input is left alone


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_small_and_large_batches(eng, tag):
    """terms = 2 at batch 1, 7 and a batch above any grid of resident workgroups, random exponents: two launches agree with each
    other and with the explicit route, and leave the key, the exponents and a alone."""
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = (16 if n == 1024 else 4) * cus + 5
    terms, w = gadget_pairs(q)[0]
    shared = plan.prepare(plan.fill_lcg(4 * terms, 77, 2))
    per_set = plan.prepare(plan.fill_lcg(big * 4 * terms, 2, 2))
    a_all = plan.fill_lcg(big * 2, 1, 2).reshape(big, 2, n)
    e_all = dev_exps(np.random.default_rng(11).integers(0, 2 ** 32, big, dtype=np.uint64).astype(np.uint32))
    before = shared.tensor.clone(), per_set.tensor.clone(), a_all.clone(), e_all.clone()
    for batch in (1, 7, big):
        a, e = a_all[:batch], e_all[:batch]
        for prepared in (shared, eng.PreparedOperand(plan, per_set.tensor[:batch * 4 * terms], batch * 4 * terms)):
            for balanced in MODES:
                c1 = plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, balanced)
                c2 = plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, balanced)
                assert torch.equal(c1, explicit(plan, a, e, prepared, terms, w, balanced)), (tag, batch, balanced)
                assert torch.equal(c1, c2), (tag, batch, balanced)
    assert torch.equal(shared.tensor, before[0]) and torch.equal(per_set.tensor, before[1]) and torch.equal(a_all, before[2])
    assert torch.equal(e_all, before[3])


def test_dynamic_row_hand_out(eng, cmux):
    """Enough output rows at n = 4096 / 60-bit, terms = 2 for plan_rows to hand rows out through the device counter: the launcher
    plans an output row with dot_row_bytes(n * 8, 2 * terms)."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w = 2, 30
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = smallest_dynamic_batch(2 * terms * n * plan.elem_bytes, resident)
    a = plan.fill_lcg(rows * 2, 1, 2).reshape(rows, 2, n); b = plan.fill_lcg(rows * 4 * terms, 2, 2)
    exps = np.random.default_rng(3).integers(0, 2 ** 32, rows, dtype=np.uint64).astype(np.uint32)
    exps[:4] = (0, n, 2 * n - 1, 1)
    e = dev_exps(exps)
    per_set, shared = plan.prepare(b), plan.prepare(b[:4 * terms])
    c = plan.poly_cmux_rotate_prepared(a, e, per_set, terms, w, True)
    assert torch.equal(c, explicit(plan, a, e, per_set, terms, w, True))
    c_shared = plan.poly_cmux_rotate_prepared(a, e, shared, terms, w, True)
    assert torch.equal(c_shared, explicit(plan, a, e, shared, terms, w, True))
    # a few rows, among them the first and last of the launch and of chunks in between, against the CPU stepping
    idx = sorted({0, 1, rows // 6 - 1, rows // 6, 1777 % rows, rows // 2 - 1, rows // 2, rows - 1})
    sel = torch.tensor(idx, device=a.device)
    ha = plan.to_host(a[sel].reshape(-1, n)).astype(np.uint64).reshape(len(idx), 2, n)
    hb = plan.to_host(per_set.tensor.reshape(rows, 4 * terms, n)[sel].reshape(-1, n)).astype(np.uint64)
    got = plan.to_host(c[sel].reshape(-1, n)).astype(np.uint64).reshape(len(idx), 2, n)
    assert np.array_equal(got, cmux.rotate(n, q, psi, ha, exps[idx], hb, terms, w, True))


def test_launch_on_a_side_stream(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w = 3, 20
    a = plan.fill_lcg(9 * 2, 5, 2).reshape(9, 2, n); b = plan.fill_lcg(9 * 4 * terms, 6, 2)
    e = dev_exps(np.array([0, 1, n - 1, n, n + 1, 2 * n - 1, 2 * n + 3, 77, 5000], dtype=np.uint32))
    per_set, shared = plan.prepare(b), plan.prepare(b[:4 * terms])
    ref = explicit(plan, a, e, per_set, terms, w, True)
    ref_shared = explicit(plan, a, e, shared, terms, w, False)
    ref_mono = plan.monomial_mul(a, e)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = plan.poly_cmux_rotate_prepared(a, e, per_set, terms, w, True, stream=side)
        c_shared = plan.poly_cmux_rotate_prepared(a, e, shared, terms, w)     # stream=None: torch's current stream, `side` here
        mono = plan.monomial_mul(a, e, stream=side)
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c_shared, ref_shared) and torch.equal(mono, ref_mono)


def test_capture_into_a_graph_sees_the_exponents_at_replay_time(eng):
    """One launch captured into a graph (one kernel node, no parallel branches) and replayed twice onto a zeroed output, the
    exponents in the captured buffer CHANGED between the replays: each replay equals the explicit route for the exponents that
    were in the buffer when it ran (the kernel reads exps, the host does not), and the two differ."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w = 2, 30
    rows = 1500
    a = plan.fill_lcg(rows * 2, 3, 2).reshape(rows, 2, n); b = plan.fill_lcg(rows * 4 * terms, 4, 2)
    prepared = plan.prepare(b)
    rng = np.random.default_rng(9)
    sets = [dev_exps(rng.integers(0, 2 ** 32, rows, dtype=np.uint64).astype(np.uint32)) for _ in range(3)]
    refs = [explicit(plan, a, e, prepared, terms, w, True) for e in sets]
    assert not torch.equal(refs[1], refs[2])
    e = sets[0].clone()
    s1 = torch.cuda.Stream(); c = torch.zeros_like(refs[0])
    torch.cuda.synchronize()          # the inputs, the references and the zero fill ran on the default stream: s1 starts behind them
    with torch.cuda.stream(s1):
        plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, True, out=c, stream=s1)     # warm-up outside the capture
    s1.synchronize()
    assert torch.equal(c, refs[0])
    g = torch.cuda.CUDAGraph(); c.zero_(); torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s1):
        plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, True, out=c, stream=s1)
    for rep in (1, 2):
        c.zero_(); e.copy_(sets[rep]); torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(c, refs[rep]), rep


def test_blind_rotate_is_three_explicit_steps(eng):
    import torch
    n, q, psi = PARAMS["P256"]
    plan = eng.get_plan(n, q, psi)
    steps, batch = 3, 6
    terms, w = gadget_pairs(q)[1]
    acc = plan.fill_lcg(batch * 2, 21, 2).reshape(batch, 2, n)
    keys = plan.prepare(plan.fill_lcg(steps * 4 * terms, 8, 2))
    exps = np.random.default_rng(4).integers(0, 2 * n, (steps, batch)).astype(np.uint32)
    exps[0, :3] = (0, n, 2 * n - 1)
    before = acc.clone()
    want = acc
    for k in range(steps):
        key = eng.PreparedOperand(plan, keys.tensor[k * 4 * terms:(k + 1) * 4 * terms], 4 * terms)
        want = explicit(plan, want, dev_exps(exps[k]), key, terms, w, True)
    got = plan.blind_rotate(acc, dev_exps(exps.reshape(-1)).reshape(steps, batch), keys, terms, w, True)
    assert torch.equal(got, want) and torch.equal(acc, before)
    assert torch.equal(plan.blind_rotate(acc, exps.tolist(), keys, terms, w, True), want)          # host exponents
    with pytest.raises(ValueError):
        plan.blind_rotate(acc, exps[:2].tolist(), keys, terms, w, True)                            # 2 steps, 3 keys


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    k = q.bit_length()
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, comps, terms, w = 5, 2, 2, 30
    a = plan.fill_lcg(batch * comps, 1, 2).reshape(batch, comps, n); b = plan.fill_lcg(batch * 4 * terms, 2, 2)
    prepared = plan.prepare(b)
    e = dev_exps(np.array([0, 1, n, 2 * n - 1, 12345], dtype=np.uint32))
    c = torch.empty((batch, comps, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, X, BH, C = a.data_ptr(), e.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr()
    row_bytes = n * plan.elem_bytes
    OK, EINVAL, EUNSUPPORTED = eng.TN_OK, eng.TN_EINVAL, eng.TN_EUNSUPPORTED
    fn, mono = lib.tn_poly_cmux_rotate_prepared_dev, lib.tn_monomial_mul_dev

    def call(p, a_, x_, bh, sets, c_, batch_, comps_, terms_, w_=w, flags=0):
        return fn(p._h, a_, x_, bh, sets, c_, batch_, comps_, terms_, w_, flags, stream)

    last = explicit(plan, a, e, prepared, terms, k - 1, False)       # what the last accepted launch into c below computes
    assert call(plan, A, X, BH, batch, C, batch, comps, terms) == OK
    assert call(plan, A, X, BH, batch, C, batch, comps, terms, w, eng.GADGET_BALANCED) == OK
    assert fn(None, A, X, BH, batch, C, batch, comps, terms, w, 0, stream) == EINVAL                  # NULL plan
    assert call(plan, None, X, BH, batch, C, batch, comps, terms) == EINVAL
    assert call(plan, A, None, BH, batch, C, batch, comps, terms) == EINVAL                         # NULL exps
    assert call(plan, A, X, None, batch, C, batch, comps, terms) == EINVAL
    assert call(plan, A, X, BH, batch, None, batch, comps, terms) == EINVAL
    assert call(plan, A, X, BH, batch, C, batch, 0, terms) == EINVAL                                # comps == 0
    for bad in (1, 3):
        assert call(plan, A, X, BH, batch, C, batch, bad, terms) == EUNSUPPORTED
        assert b"tn_monomial_mul_dev, tn_poly_external_product_prepared_dev" in lib.tn_last_error()
    assert call(plan, A, X, BH, batch, C, batch, comps, 0) == EINVAL                                # terms == 0
    assert call(plan, A, X, BH, batch, C, batch, comps, terms, 0) == EINVAL                         # base_log == 0
    assert call(plan, A, X, BH, batch, C, batch, comps, terms, k) == EINVAL                         # 2^base_log >= q
    assert call(plan, A, X, BH, batch, C, batch, comps, 4, 22) == EINVAL                            # (terms - 1) * base_log = 66
    assert call(plan, A, X, BH, batch, C, batch, comps, terms, w, 2) == EINVAL                      # an unknown flag bit
    assert call(plan, A, X, BH, 2, C, batch, comps, terms) == EINVAL                                # neither 1 nor batch
    assert call(plan, A, X, BH, batch, A, batch, comps, terms) == EINVAL                            # c is a: no run in place
    assert call(plan, A, X, BH, batch, BH, batch, comps, terms) == EINVAL                           # c is bhat
    assert call(plan, A, X, BH, batch, A + (batch * comps - 1) * row_bytes, batch, comps, terms) == EINVAL      # c's first row is a's last
    assert call(plan, A, X, BH, batch, A - (batch * comps - 1) * row_bytes, batch, comps, terms) == EINVAL      # c's last row is a's first
    assert call(plan, A, X, BH, 1, BH + (4 * terms - 1) * row_bytes, batch, comps, terms) == EINVAL            # ... the shared key's last
    assert call(plan, A, X, BH, batch, C, batch, comps, terms, k - 1) == OK                         # 2^(k-1) < q, one shift of k - 1
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_terms, w_ in ((2 ** 29, 1, 30), (2 ** 28, 2, 30), (2 ** 24, 32, 2), (2 ** 63, 1, 30)):
        assert call(plan, dummy, dummy, dummy, 1, dummy, big_batch, comps, big_terms, w_) == EINVAL, (big_batch, big_terms)
        assert b"batch * comps * comps * terms too large" in lib.tn_last_error()
    assert call(plan, None, None, None, 1, None, 0, comps, 3, 20) == OK                             # batch 0 launches nothing
    torch.cuda.synchronize()
    assert torch.equal(c, last)

    # the monomial call through the C ABI
    m = torch.empty_like(a); M = m.data_ptr()
    assert mono(plan._h, A, X, M, batch, comps, eng.MONOMIAL_MINUS_ONE, stream) == OK
    want = plan.monomial_mul(a, e, True)
    assert mono(None, A, X, M, batch, comps, 0, stream) == EINVAL
    assert mono(plan._h, A, X, M, batch, 0, 0, stream) == EINVAL and b"group must be at least 1" in lib.tn_last_error()
    assert mono(plan._h, A, X, M, batch, comps, 2, stream) == EINVAL and b"unknown flag bit" in lib.tn_last_error()
    assert mono(plan._h, dummy, dummy, dummy, 2 ** 30, 2, 0, stream) == EINVAL and b"batch * group too large" in lib.tn_last_error()
    assert mono(plan._h, None, None, None, 0, comps, 0, stream) == OK
    assert mono(plan._h, None, X, M, batch, comps, 0, stream) == EINVAL
    assert mono(plan._h, A, None, M, batch, comps, 0, stream) == EINVAL
    assert mono(plan._h, A, X, None, batch, comps, 0, stream) == EINVAL
    assert mono(plan._h, A, X, A, batch, comps, 0, stream) == EINVAL and b"overlap the input" in lib.tn_last_error()
    assert mono(plan._h, A, X, A + (batch * comps - 1) * row_bytes, batch, comps, 0, stream) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(m, want)

    # plans without the fused kernels refuse the fused call: a general plan, an omega-only plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    for other in others:
        assert not other.has_fused
        x = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty((16, other.n), dtype=other.torch_dtype, device="cuda:0")
        z = torch.empty_like(x)
        assert call(other, x.data_ptr(), X, y.data_ptr(), 1, z.data_ptr(), 2, 2, 2) == EUNSUPPORTED
        assert b"fused kernels" in lib.tn_last_error()

    # the Python side
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_cmux_rotate_prepared(a, e, prepared, terms, w)
    with pytest.raises(TypeError):
        plan.poly_cmux_rotate_prepared(a, e, b, terms, w)
    with pytest.raises(ValueError):
        plan.poly_cmux_rotate_prepared(a, e, plan.prepare(b[:3]), terms, w)           # 3 rows: neither one key nor batch keys
    with pytest.raises(ValueError):
        plan.poly_cmux_rotate_prepared(a.reshape(-1), e, prepared, terms, w)          # a needs (batch, 2, n) or (2, n)
    with pytest.raises(ValueError):
        plan.poly_cmux_rotate_prepared(a[:, :, :n - 1], e, prepared, terms, w)
    with pytest.raises(eng.TinyNttError):
        plan.poly_cmux_rotate_prepared(a[:, :1], e, plan.prepare(b[:terms]), terms, w)      # a view that is not contiguous
    with pytest.raises(eng.TinyNttError, match="comps other than 2"):
        plan.poly_cmux_rotate_prepared(a.reshape(batch * 2, 1, n), dev_exps(np.zeros(batch * 2)), plan.prepare(b[:terms]), terms, w)
    with pytest.raises(ValueError):
        plan.poly_cmux_rotate_prepared(a, e[:3], prepared, terms, w)                   # 3 exponents for 5 rows
    with pytest.raises(eng.TinyNttError):
        plan.poly_cmux_rotate_prepared(a, e.to(torch.int64), prepared, terms, w)       # exponents are 32-bit words
    with pytest.raises(eng.TinyNttError):
        plan.poly_cmux_rotate_prepared(a, e.cpu(), prepared, terms, w)                 # a torch tensor on the host
    with pytest.raises(TypeError):
        plan.poly_cmux_rotate_prepared(a, [0.5] * batch, prepared, terms, w)
    with pytest.raises(eng.TinyNttError, match="overlap"):
        plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, out=a)                # in place is out of scope
    # out is checked like poly_external_product_prepared's: a host tensor or another word size never reaches the kernel
    with pytest.raises(eng.TinyNttError):
        plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, out=torch.empty((batch, comps, n), dtype=plan.torch_dtype))
    with pytest.raises(eng.TinyNttError):
        plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, out=torch.empty((batch, comps, n), dtype=torch.int32, device=a.device))
    with pytest.raises(ValueError):
        plan.poly_cmux_rotate_prepared(a, e, prepared, terms, w, out=torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            plan.poly_cmux_rotate_prepared(a, e, prepared, bad, w)
    with pytest.raises(ValueError):
        plan.monomial_mul(a.reshape(-1), e)
    with pytest.raises(ValueError):
        plan.monomial_mul(a, e[:2])
    with pytest.raises(eng.TinyNttError, match="overlap"):
        plan.monomial_mul(a, e, out=a)
    torch.cuda.synchronize()
    assert torch.equal(c, last)
