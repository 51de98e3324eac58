"""GPU tests of tn_poly_blind_rotate_prepared_dev (Plan.poly_blind_rotate_prepared): a blind rotation from one launch with the
accumulator in LDS across the steps, bit for bit against the loop it replaces on the device (Plan.blind_rotate: one
tn_poly_cmux_rotate_prepared_dev launch per step over two alternating buffers), against the CPU stepping of the kernel
(tests/emu/emu_blindrot.cpp) and against an algebraic identity that does not pass through the project's decomposition."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from test_blindrot_emu import BATCH, STEPS, EmuBlindrot, step_exponents, step_key_rows
from test_cmux_emu import TRIVIAL, monomial_np, trivial_key
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu
FN, LOOP = "tn_poly_blind_rotate_prepared_dev", b"tn_poly_cmux_rotate_prepared_dev"


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def blindrot():
    return EmuBlindrot()


def dev_exps(exps):
    """(steps, batch) of any 32-bit words -> a device tensor of that shape."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(exps, dtype=np.uint32).view(np.int32)).to("cuda:0")


def supported(blindrot, plan):
    return blindrot.lds(plan.n, plan.elem_bytes, plan.is_lazy)[0]


def check_parity(plan, blindrot, n, q, psi, a, b, canonical):
    """Batch 7, three steps, every (terms, w) of gadget_pairs, both digit modes: torch.equal with the loop on the device; for one
    pair, also the CPU stepping."""
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)
    exps = step_exponents(n, STEPS)
    de = dev_exps(exps)
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        ha = np.ascontiguousarray(a[input_rows(BATCH, 2, first)])            # (7, 2, n)
        da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
        keys = plan.prepare(b[step_key_rows(STEPS, terms).ravel()])
        assert keys.rows == STEPS * 4 * terms
        for balanced in MODES:
            where = (terms, w, balanced)
            c = plan.poly_blind_rotate_prepared(da, de, keys, terms, w, balanced)
            assert c.shape == (BATCH, 2, n) and c.data_ptr() != da.data_ptr()
            assert torch.equal(c, plan.blind_rotate(da, de, keys, terms, w, balanced)), where
            if first == 1:
                bhat = plan.to_host(keys.tensor).astype(np.uint64)
                hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
                assert np.array_equal(hc, blindrot.rotate(n, q, psi, ha, exps, bhat, terms, w, balanced, canonical)), where


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_one_launch_equals_the_loop_and_the_stepping(eng, blindrot, case):
    import torch
    n, q, psi, a, b = _case_data(case)
    plan = eng.get_plan(n, q, psi)
    if supported(blindrot, plan):
        check_parity(plan, blindrot, n, q, psi, a, b, False)
        return
    # a shape whose accumulator does not fit: TN_EUNSUPPORTED, the text names the loop, c is left as it was
    assert case == "P8192_60"
    terms, w = gadget_pairs(q)[0]
    da = plan.to_device(np.array(a)[input_rows(2, 2)].reshape(4, n)).reshape(2, 2, n)
    keys = plan.prepare(np.array(b)[step_key_rows(1, terms).ravel()])
    de = dev_exps(step_exponents(n, 1, 2))
    c = torch.full_like(da, 5)
    st = plan._lib.tn_poly_blind_rotate_prepared_dev(plan._h, da.data_ptr(), de.data_ptr(), keys.tensor.data_ptr(), c.data_ptr(), 2, 2, 1, terms, w, 0,
                                                     plan._stream_ptr(None))
    assert st == eng.TN_EUNSUPPORTED and LOOP in plan._lib.tn_last_error()
    with pytest.raises(eng.TinyNttError, match="tn_poly_cmux_rotate_prepared_dev"):
        plan.poly_blind_rotate_prepared(da, de, keys, terms, w, out=c)
    torch.cuda.synchronize()
    assert torch.equal(c, torch.full_like(da, 5))
    assert plan.blind_rotate(da, de, keys, terms, w).shape == (2, 2, n)          # the loop runs at this shape


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_on_a_canonical_policy_plan(eng, blindrot, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(plan, blindrot, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag,steps", [("P256", 9), ("P1024", 4)])
def test_trivial_rgsw_keys_of_bits_rotate_by_the_selected_sum(eng, tag, steps):
    """Noise-free trivial RGSW keys of bits m_k with unsigned digits that cover q (tests/test_cmux_emu.py): the launch returns
    rot_E(a mod q), E = sum m_k e_k mod 2n, word for word; nothing here passes through the project's decomposition."""
    n, q, psi, a, _ = _case_data(tag)
    plan = eng.get_plan(n, q, psi)
    terms, w = TRIVIAL[q.bit_length()]
    bits = np.random.default_rng(n).integers(0, 2, steps)
    bits[0], bits[1] = 1, 0
    keys = plan.prepare(np.concatenate([trivial_key(n, q, int(m), terms, w) for m in bits]))
    exps = step_exponents(n, steps)
    ha = np.ascontiguousarray(np.array(a)[input_rows(BATCH, 2)])
    da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
    total = [sum(int(bits[k]) * int(exps[k, r]) for k in range(steps)) % (2 * n) for r in range(BATCH)]
    c = plan.poly_blind_rotate_prepared(da, dev_exps(exps), keys, terms, w)
    assert np.array_equal(plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n), monomial_np(ha, total, q)), tag


def test_batches_repeatability_and_in_place(eng):
    """Batch 1, batch 7 and more rows than workgroups can be resident (a workgroup reloads the LDS accumulator for a second row) at
    P1024 with two steps, both digit modes: two launches agree with each other and with the loop and leave a, the exponents and
    the keys alone; then out=acc gives the bits of the out-of-place call."""
    import torch
    n, q, psi = PARAMS["P1024"]
    plan = eng.get_plan(n, q, psi)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = 16 * cus + 5                           # 16 workgroups of 2 waves fill a CU's wave slots: more than LDS lets be resident
    steps = 2
    terms, w = gadget_pairs(q)[0]
    keys = plan.prepare(plan.fill_lcg(steps * 4 * terms, 77, 2))
    a_all = plan.fill_lcg(big * 2, 1, 2).reshape(big, 2, n)
    e_np = np.random.default_rng(11).integers(0, 2 ** 32, (steps, big), dtype=np.uint64).astype(np.uint32)
    before_keys, before_a = keys.tensor.clone(), a_all.clone()
    for batch in (1, 7, big):
        a, e = a_all[:batch], dev_exps(e_np[:, :batch])
        before_e = e.clone()
        for balanced in MODES:
            c1 = plan.poly_blind_rotate_prepared(a, e, keys, terms, w, balanced)
            c2 = plan.poly_blind_rotate_prepared(a, e, keys, terms, w, balanced)
            assert torch.equal(c1, plan.blind_rotate(a, e, keys, terms, w, balanced)), (batch, balanced)
            assert torch.equal(c1, c2), (batch, balanced)
        assert torch.equal(e, before_e)
        acc = a.clone()
        got = plan.poly_blind_rotate_prepared(acc, e, keys, terms, w, MODES[-1], out=acc)
        assert got.data_ptr() == acc.data_ptr() and torch.equal(acc, c1), batch
    assert torch.equal(keys.tensor, before_keys) and torch.equal(a_all, before_a)


def test_launch_on_a_side_stream(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w, steps, batch = 3, 20, 2, 9
    a = plan.fill_lcg(batch * 2, 5, 2).reshape(batch, 2, n)
    keys = plan.prepare(plan.fill_lcg(steps * 4 * terms, 6, 2))
    e = dev_exps(step_exponents(n, steps, batch))
    ref = plan.blind_rotate(a, e, keys, terms, w, True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = plan.poly_blind_rotate_prepared(a, e, keys, terms, w, True, stream=side)
        c2 = plan.poly_blind_rotate_prepared(a, e, keys, terms, w, True)        # stream=None: torch's current stream, `side` here
    side.synchronize()
    assert torch.equal(c, ref) and torch.equal(c2, ref)


def test_capture_into_a_graph_sees_the_exponents_at_replay_time(eng):
    """One launch captured into a graph (one kernel node, no parallel branches) and replayed twice onto a zeroed output, the
    exponents in the captured buffer CHANGED between the replays: each replay equals the loop for the exponents that were in the
    buffer when it ran (the kernel reads exps, the host does not), and the two differ."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w, steps, rows = 2, 30, 3, 600
    a = plan.fill_lcg(rows * 2, 3, 2).reshape(rows, 2, n)
    keys = plan.prepare(plan.fill_lcg(steps * 4 * terms, 4, 2))
    rng = np.random.default_rng(9)
    sets = [dev_exps(rng.integers(0, 2 ** 32, (steps, rows), dtype=np.uint64).astype(np.uint32)) for _ in range(3)]
    refs = [plan.blind_rotate(a, e, keys, terms, w, True) for e in sets]
    assert not torch.equal(refs[1], refs[2])
    e = sets[0].clone()
    s1 = torch.cuda.Stream(); c = torch.zeros_like(refs[0])
    torch.cuda.synchronize()          # the inputs, the references and the zero fill ran on the default stream: s1 starts behind them
    with torch.cuda.stream(s1):
        plan.poly_blind_rotate_prepared(a, e, keys, terms, w, True, out=c, stream=s1)      # warm-up outside the capture
    s1.synchronize()
    assert torch.equal(c, refs[0])
    g = torch.cuda.CUDAGraph(); c.zero_(); torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=s1):
        plan.poly_blind_rotate_prepared(a, e, keys, terms, w, True, out=c, stream=s1)
    for rep in (1, 2):
        c.zero_(); e.copy_(sets[rep]); torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            g.replay()
        torch.cuda.synchronize()
        assert torch.equal(c, refs[rep]), rep


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    k = q.bit_length()
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, comps, steps, terms, w = 5, 2, 3, 2, 30
    a = plan.fill_lcg(batch * comps, 1, 2).reshape(batch, comps, n)
    keys = plan.prepare(plan.fill_lcg(steps * 4 * terms, 2, 2))
    e = dev_exps(step_exponents(n, steps, batch))
    c = torch.empty((batch, comps, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, X, BH, C = a.data_ptr(), e.data_ptr(), keys.tensor.data_ptr(), c.data_ptr()
    row_bytes = n * plan.elem_bytes
    OK, EINVAL, EUNSUPPORTED = eng.TN_OK, eng.TN_EINVAL, eng.TN_EUNSUPPORTED
    fn = lib.tn_poly_blind_rotate_prepared_dev

    def call(p, a_, x_, bh, c_, batch_, comps_, steps_, terms_, w_=w, flags=0):
        return fn(p._h, a_, x_, bh, c_, batch_, comps_, steps_, terms_, w_, flags, stream)

    last = plan.blind_rotate(a, e, keys, terms, k - 1, False)        # what the last accepted launch into c below computes
    assert call(plan, A, X, BH, C, batch, comps, steps, terms) == OK
    assert call(plan, A, X, BH, C, batch, comps, steps, terms, w, eng.GADGET_BALANCED) == OK
    assert fn(None, A, X, BH, C, batch, comps, steps, terms, w, 0, stream) == EINVAL                # NULL plan
    assert call(plan, None, X, BH, C, batch, comps, steps, terms) == EINVAL
    assert call(plan, A, None, BH, C, batch, comps, steps, terms) == EINVAL                         # NULL exps
    assert call(plan, A, X, None, C, batch, comps, steps, terms) == EINVAL
    assert call(plan, A, X, BH, None, batch, comps, steps, terms) == EINVAL
    assert call(plan, A, X, BH, C, batch, 0, steps, terms) == EINVAL                                # comps == 0
    for bad in (1, 3):
        assert call(plan, A, X, BH, C, batch, bad, steps, terms) == EUNSUPPORTED
        assert b"comps other than 2" in lib.tn_last_error()
    assert call(plan, A, X, BH, C, batch, comps, 0, terms) == EINVAL and b"steps must be at least 1" in lib.tn_last_error()
    assert call(plan, A, X, BH, C, batch, comps, steps, 0) == EINVAL                                # terms == 0
    assert call(plan, A, X, BH, C, batch, comps, steps, terms, 0) == EINVAL                         # base_log == 0
    assert call(plan, A, X, BH, C, batch, comps, steps, terms, k) == EINVAL                         # 2^base_log >= q
    assert call(plan, A, X, BH, C, batch, comps, steps, 4, 22) == EINVAL                            # (terms - 1) * base_log = 66
    assert call(plan, A, X, BH, C, batch, comps, steps, terms, w, 2) == EINVAL                      # an unknown flag bit
    assert call(plan, A, X, BH, BH, batch, comps, steps, terms) == EINVAL                           # c is bhat
    assert b"overlap the key" in lib.tn_last_error()
    assert call(plan, A, X, BH, BH + (steps * 4 * terms - 1) * row_bytes, batch, comps, steps, terms) == EINVAL     # ... the last key's last row
    assert call(plan, A, X, BH, A + row_bytes, batch, comps, steps, terms) == EINVAL                # c overlaps a and is not a
    assert b"c may be a itself" in lib.tn_last_error()
    assert call(plan, A, X, BH, A - (batch * comps - 1) * row_bytes, batch, comps, steps, terms) == EINVAL          # c's last row is a's first
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_steps, big_terms, text in ((1, 2 ** 29, 1, b"steps * 4 * terms too large"), (2 ** 30, 1, 1, b"batch * 2 too large"),
                                                  (2 ** 16, 2 ** 15, 1, b"steps * batch too large"), (2 ** 63, 1, 1, b"batch * 2 too large")):
        assert call(plan, dummy, dummy, dummy, dummy, big_batch, comps, big_steps, big_terms, 30) == EINVAL, (big_batch, big_steps)
        assert text in lib.tn_last_error()
    assert call(plan, None, None, None, None, 0, comps, steps, 3, 20) == OK                         # batch 0 launches nothing
    assert call(plan, A, X, BH, C, batch, comps, steps, terms, k - 1) == OK                         # 2^(k-1) < q, one shift of k - 1
    torch.cuda.synchronize()
    assert torch.equal(c, last)

    # plans without the fused kernels refuse the call: a general plan, an omega-only plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    for other in others:
        assert not other.has_fused
        x = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty((16, other.n), dtype=other.torch_dtype, device="cuda:0")
        z = torch.empty_like(x)
        assert call(other, x.data_ptr(), X, y.data_ptr(), z.data_ptr(), 2, 2, 2, 2) == EUNSUPPORTED
        assert b"fused kernels" in lib.tn_last_error()

    # the Python side
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_blind_rotate_prepared(a, e, keys, terms, w)
    with pytest.raises(TypeError):
        plan.poly_blind_rotate_prepared(a, e, keys.tensor, terms, w)
    with pytest.raises(ValueError):
        plan.poly_blind_rotate_prepared(a, e[:2], keys, terms, w)                     # 2 steps, 3 keys
    with pytest.raises(ValueError):
        plan.poly_blind_rotate_prepared(a, e[:, :3].contiguous(), keys, terms, w)     # 3 exponents per step for 5 rows
    with pytest.raises(ValueError):
        plan.poly_blind_rotate_prepared(a.reshape(-1, n), e, keys, terms, w)          # acc needs (batch, 2, n)
    with pytest.raises(ValueError):
        plan.poly_blind_rotate_prepared(plan.to_host(a.reshape(-1, n)).reshape(batch, comps, n), e, keys, terms, w)      # a host array
    with pytest.raises(eng.TinyNttError):
        plan.poly_blind_rotate_prepared(a[:, :1], e, keys, terms, w)                  # a view that is not contiguous
    with pytest.raises(eng.TinyNttError):
        plan.poly_blind_rotate_prepared(a, e.to(torch.int64), keys, terms, w)         # exponents are 32-bit words
    with pytest.raises(eng.TinyNttError):
        plan.poly_blind_rotate_prepared(a, e.cpu(), keys, terms, w)                   # a torch tensor on the host
    with pytest.raises(TypeError):
        plan.poly_blind_rotate_prepared(a, [[0.5] * batch] * steps, keys, terms, w)
    with pytest.raises(eng.TinyNttError, match="c may be a itself"):
        plan.poly_blind_rotate_prepared(a[:2], e[:, :2].contiguous(), keys, terms, w, out=a[1:3])       # overlaps a and is not a
    with pytest.raises(eng.TinyNttError):
        plan.poly_blind_rotate_prepared(a, e, keys, terms, w, out=torch.empty((batch, comps, n), dtype=plan.torch_dtype))
    with pytest.raises(eng.TinyNttError):
        plan.poly_blind_rotate_prepared(a, e, keys, terms, w, out=torch.empty((batch, comps, n), dtype=torch.int32, device=a.device))
    with pytest.raises(ValueError):
        plan.poly_blind_rotate_prepared(a, e, keys, terms, w, out=torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            plan.poly_blind_rotate_prepared(a, e, keys, bad, w)
    host = plan.poly_blind_rotate_prepared(a, step_exponents(n, steps, batch).astype(np.int64) + 4 * n, keys, terms, w)      # host exponents of any size
    assert torch.equal(host, plan.blind_rotate(a, e, keys, terms, w))
    torch.cuda.synchronize()
    assert torch.equal(c, last)
