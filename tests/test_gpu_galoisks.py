"""GPU tests of tn_poly_galois_keyswitch_prepared_dev (Plan.poly_galois_keyswitch_prepared): the homomorphic automorphism of an RLWE
ciphertext from one launch, bit for bit against the explicit route on the device (tn_automorphism_dev on both components,
tn_poly_gadget_multidot_prepared_dev with outs = 2 on the rotated second one, the addition mod q) and against the CPU stepping
of the kernel (tests/emu_galoisks/emu_galoisks.cpp); with a trivial key against the numpy statement of sigma_g."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_cmux_emu import TRIVIAL
from test_extprod_emu import input_rows
from test_gadget_emu import MODES, gadget_pairs
from test_galoisks_emu import BATCH, EmuGaloisKs, elements, key_rows, trivial_key, trivial_want
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def ks():
    return EmuGaloisKs()


def explicit(plan, a, g, prepared, terms, w, balanced):
    """The contract: automorphism on a viewed as batch * 2 rows, poly_gadget_multidot_prepared with outs = 2 on the rotated
    a[r][1] rows, component 0 plus the rotated a[r][0] mod q (both canonical: the sum is taken in 64 bits, q < 2^62)."""
    import torch
    n = plan.n
    rot = plan.automorphism(a.reshape(-1, n), int(g)).reshape(-1, 2, n)
    c = plan.poly_gadget_multidot_prepared(rot[:, 1].contiguous(), prepared, 2, terms, w, balanced)
    s = c[:, 0].to(torch.int64) + rot[:, 0].to(torch.int64)
    c[:, 0] = torch.where(s >= plan.q, s - plan.q, s).to(plan.torch_dtype)
    return c


def check_parity(eng, plan, ks, n, q, psi, a, b, canonical):
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        ha = np.ascontiguousarray(a[input_rows(BATCH, 2, first)])            # (7, 2, n)
        da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
            assert prepared.rows == (2 * terms if shared else BATCH * 2 * terms)
            bhat = plan.to_host(prepared.tensor).astype(np.uint64)
            for balanced in MODES:
                for g in elements(n):
                    where = (terms, w, shared, balanced, g)
                    c = plan.poly_galois_keyswitch_prepared(da, g, prepared, terms, w, balanced)
                    assert c.shape == (BATCH, 2, n)
                    assert torch.equal(c, explicit(plan, da, g, prepared, terms, w, balanced)), where
                    hc = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
                    assert np.array_equal(hc, ks.keyswitch(n, q, psi, ha, g, bhat, terms, w, balanced, canonical)), where


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_key_switch_equals_the_explicit_route_and_the_stepping(eng, ks, case):
    n, q, psi, a, b = _case_data(case)
    plan = eng.get_plan(n, q, psi)
    check_parity(eng, plan, ks, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_key_switch_on_a_canonical_policy_plan(eng, ks, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(eng, plan, ks, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_host_arrays_and_one_ciphertext(eng, tag):
    """Host arrays in, host arrays out; one ciphertext: (2, n) in, (2, n) out, from the host and from the device."""
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi)
    terms, w = gadget_pairs(q)[1]
    g = n + 1
    ha = np.array(a)[input_rows(BATCH, 2)]
    da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
    prepared = plan.prepare(np.array(b)[key_rows(1, terms, True)[0].ravel()])
    ref = plan.to_host(explicit(plan, da, g, prepared, terms, w, True).reshape(-1, n)).reshape(BATCH, 2, n)
    hc = plan.poly_galois_keyswitch_prepared(ha, g, prepared, terms, w, True)
    assert isinstance(hc, np.ndarray) and hc.shape == (BATCH, 2, n) and np.array_equal(hc, ref)
    one = plan.poly_galois_keyswitch_prepared(ha[2], g, prepared, terms, w, True)
    assert isinstance(one, np.ndarray) and one.shape == (2, n) and np.array_equal(one, ref[2])
    one = plan.poly_galois_keyswitch_prepared(da[2], g, prepared, terms, w, True)
    assert one.shape == (2, n) and np.array_equal(plan.to_host(one), ref[2])


@pytest.mark.parametrize("tag", ["P256", "P1024", "P4096_60"])
def test_trivial_key_returns_sigma_of_both_components(eng, tag):
    """Unsigned digits that cover q (tests/test_galoisks_emu.py): K[1][j] = 2^(j w) gives (sigma_g(a0), sigma_g(a1)), K[0][j] =
    2^(j w) gives (sigma_g(a0) + sigma_g(a1), 0), word for word against the numpy statement of sigma_g; nothing here passes through
    the project's decomposition or its automorphism."""
    n, q, psi, a, _ = _case_data(tag)
    plan = eng.get_plan(n, q, psi)
    terms, w = TRIVIAL[q.bit_length()]
    ha = np.ascontiguousarray(np.array(a)[input_rows(BATCH, 2)])
    da = plan.to_device(ha.reshape(BATCH * 2, n)).reshape(BATCH, 2, n)
    for component in (0, 1):
        prepared = plan.prepare(trivial_key(n, q, component, terms, w))
        for g in elements(n):
            c = plan.poly_galois_keyswitch_prepared(da, g, prepared, terms, w)
            got = plan.to_host(c.reshape(-1, n)).astype(np.uint64).reshape(BATCH, 2, n)
            assert np.array_equal(got, trivial_want(ha, g, q, component)), (tag, component, g)


@pytest.mark.parametrize("fewer", [0, 1], ids=["dynamic", "one-row-fewer"])
def test_row_hand_out(eng, ks, fewer):
    """The smallest batch at n = 4096 / 60-bit, terms = 2 that plan_rows hands out through the device counter (the launcher plans
    an output row as the two-component gadget kernel does: dot_row_bytes, terms * n * 8 bytes), and one row fewer, which keeps
    the fixed stride."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w, g = 2, 30, 2 * n - 1
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = smallest_dynamic_batch(terms * n * plan.elem_bytes, resident) - fewer
    a = plan.fill_lcg(rows * 2, 1, 2).reshape(rows, 2, n); b = plan.fill_lcg(rows * 2 * terms, 2, 2)
    per_set, shared = plan.prepare(b), plan.prepare(b[:2 * terms])
    before = a.clone()
    c = plan.poly_galois_keyswitch_prepared(a, g, per_set, terms, w, True)
    assert torch.equal(c, explicit(plan, a, g, per_set, terms, w, True))
    c_shared = plan.poly_galois_keyswitch_prepared(a, 5, shared, terms, w, True)
    assert torch.equal(c_shared, explicit(plan, a, 5, shared, terms, w, True))
    assert torch.equal(a, before)
    # a few rows, among them the first and last of the launch and of chunks in between, against the CPU stepping
    idx = sorted({0, 1, rows // 6 - 1, rows // 6, 1777 % rows, rows // 2 - 1, rows // 2, rows - 1})
    sel = torch.tensor(idx, device=a.device)
    ha = plan.to_host(a[sel].reshape(-1, n)).astype(np.uint64).reshape(len(idx), 2, n)
    hb = plan.to_host(per_set.tensor.reshape(rows, 2 * terms, n)[sel].reshape(-1, n)).astype(np.uint64)
    got = plan.to_host(c[sel].reshape(-1, n)).astype(np.uint64).reshape(len(idx), 2, n)
    assert np.array_equal(got, ks.keyswitch(n, q, psi, ha, g, hb, terms, w, True))


def test_capture_into_a_graph_replays_the_captured_element_on_new_words(eng):
    """One launch captured into a graph (one kernel node, no parallel branches) and replayed twice onto a zeroed output, a CHANGED
    in place between the replays: each replay equals a direct launch on the words that were in a when it ran, with the Galois
    element the launch was captured with (it travels by value)."""
    import torch
    n, q, psi = PARAMS["P1024"]
    plan = eng.get_plan(n, q, psi)
    terms, w = gadget_pairs(q)[0]
    rows, g = 300, n + 1
    prepared = plan.prepare(plan.fill_lcg(rows * 2 * terms, 4, 2))
    sets = [plan.fill_lcg(rows * 2, seed, 2).reshape(rows, 2, n) for seed in (3, 5, 7)]
    refs = [plan.poly_galois_keyswitch_prepared(x, g, prepared, terms, w, True) for x in sets]
    assert torch.equal(refs[0], explicit(plan, sets[0], g, prepared, terms, w, True)) and not torch.equal(refs[1], refs[2])
    a = sets[0].clone()
    s1 = torch.cuda.Stream(); c = torch.zeros_like(refs[0])
    torch.cuda.synchronize()          # the inputs, the references and the zero fill ran on the default stream: s1 starts behind them
    with torch.cuda.stream(s1):
        plan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w, True, out=c, stream=s1)     # warm-up outside the capture
    s1.synchronize()
    assert torch.equal(c, refs[0])
    graph = torch.cuda.CUDAGraph(); c.zero_(); torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s1):
        plan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w, True, out=c, stream=s1)
    for rep in (1, 2):
        c.zero_(); a.copy_(sets[rep]); torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c, refs[rep]), rep


def test_status_codes(eng):
    import torch
    n, q, psi = PARAMS["P4096_60"]
    k = q.bit_length()
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, terms, w, g = 5, 2, 30, 3
    a = plan.fill_lcg(batch * 2, 1, 2).reshape(batch, 2, n); b = plan.fill_lcg(batch * 2 * terms, 2, 2)
    prepared = plan.prepare(b)
    c = torch.empty((batch, 2, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, BH, C = a.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr()
    row_bytes = n * plan.elem_bytes
    OK, EINVAL, EUNSUPPORTED = eng.TN_OK, eng.TN_EINVAL, eng.TN_EUNSUPPORTED
    fn = lib.tn_poly_galois_keyswitch_prepared_dev

    def call(p, a_, g_, bh, sets, c_, batch_, terms_, w_=w, flags=0):
        return fn(p._h, a_, g_, bh, sets, c_, batch_, terms_, w_, flags, stream)

    last = explicit(plan, a, g, prepared, terms, k - 1, False)       # what the last accepted launch into c below computes
    assert call(plan, A, g, BH, batch, C, batch, terms) == OK
    assert call(plan, A, g, BH, batch, C, batch, terms, w, eng.GADGET_BALANCED) == OK
    assert fn(None, A, g, BH, batch, C, batch, terms, w, 0, stream) == EINVAL                  # NULL plan
    for bad in (0, 4, 2 * n, 2 * n + 1, 2 ** 32 - 1):
        assert call(plan, A, bad, BH, batch, C, batch, terms) == EINVAL, bad
        assert b"is not an odd element below 2n" in lib.tn_last_error()
    assert call(plan, None, g, BH, batch, C, batch, terms) == EINVAL
    assert call(plan, A, g, None, batch, C, batch, terms) == EINVAL
    assert call(plan, A, g, BH, batch, None, batch, terms) == EINVAL
    assert call(plan, A, g, BH, batch, C, batch, 0) == EINVAL                                # terms == 0
    assert call(plan, A, g, BH, batch, C, batch, terms, 0) == EINVAL                         # base_log == 0
    assert call(plan, A, g, BH, batch, C, batch, terms, k) == EINVAL                         # 2^base_log >= q
    assert call(plan, A, g, BH, batch, C, batch, 4, 22) == EINVAL                            # (terms - 1) * base_log = 66
    assert call(plan, A, g, BH, batch, C, batch, terms, w, 2) == EINVAL                      # an unknown flag bit
    assert call(plan, A, g, BH, 2, C, batch, terms) == EINVAL                                # neither 1 nor batch
    assert call(plan, A, g, BH, batch, A, batch, terms) == EINVAL                            # c is a: no run in place
    assert call(plan, A, g, BH, batch, BH, batch, terms) == EINVAL                           # c is bhat
    assert call(plan, A, g, BH, batch, A + (batch * 2 - 1) * row_bytes, batch, terms) == EINVAL      # c's first row is a's last
    assert call(plan, A, g, BH, batch, A - (batch * 2 - 1) * row_bytes, batch, terms) == EINVAL      # c's last row is a's first
    assert call(plan, A, g, BH, 1, BH + (2 * terms - 1) * row_bytes, batch, terms) == EINVAL        # ... the shared key's last
    assert call(plan, A, g, BH, batch, C, batch, terms, k - 1) == OK                         # 2^(k-1) < q, one shift of k - 1
    dummy = ctypes.c_void_p(4096)
    for big_batch, big_terms, w_ in ((2 ** 30, 1, 30), (2 ** 29, 2, 30), (2 ** 25, 32, 1), (2 ** 63, 1, 30)):
        assert call(plan, dummy, g, dummy, 1, dummy, big_batch, big_terms, w_) == EINVAL, (big_batch, big_terms)
        assert b"batch * 2 * terms too large" in lib.tn_last_error()
    assert call(plan, None, g, None, 1, None, 0, 3, 20) == OK                                # batch 0 launches nothing
    torch.cuda.synchronize()
    assert torch.equal(c, last)

    # plans without the fused kernels refuse the call: a general plan, an omega-only plan and n = 16
    small_psi = next(p for p in (pow(x, (q - 1) // 32, q) for x in range(2, 500)) if pow(p, 16, q) == q - 1)
    others = [eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q)), eng.get_plan(16, q, small_psi)]
    for other in others:
        assert not other.has_fused
        x = torch.zeros((4, other.n), dtype=other.torch_dtype, device="cuda:0"); y = torch.empty((8, other.n), dtype=other.torch_dtype, device="cuda:0")
        z = torch.empty_like(x)
        assert call(other, x.data_ptr(), g, y.data_ptr(), 1, z.data_ptr(), 2, 2) == EUNSUPPORTED
        assert b"fused kernels" in lib.tn_last_error()

    # the Python side
    cplan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        cplan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w)
    with pytest.raises(TypeError):
        plan.poly_galois_keyswitch_prepared(a, g, b, terms, w)
    with pytest.raises(ValueError):
        plan.poly_galois_keyswitch_prepared(a, g, plan.prepare(b[:3]), terms, w)           # 3 rows: neither one key nor batch keys
    with pytest.raises(ValueError):
        plan.poly_galois_keyswitch_prepared(a.reshape(-1), g, prepared, terms, w)          # a needs (batch, 2, n) or (2, n)
    with pytest.raises(ValueError):
        plan.poly_galois_keyswitch_prepared(a.reshape(batch * 2, 1, n), g, prepared, terms, w)
    with pytest.raises(ValueError):
        plan.poly_galois_keyswitch_prepared(a[:, :, :n - 1], g, prepared, terms, w)
    with pytest.raises(eng.TinyNttError):
        plan.poly_galois_keyswitch_prepared(a[::2], g, plan.prepare(b[:2 * terms]), terms, w)      # a view that is not contiguous
    for bad in (2, 2 * n + 1):
        with pytest.raises(eng.TinyNttError, match="odd element below 2n"):
            plan.poly_galois_keyswitch_prepared(a, bad, prepared, terms, w)
    with pytest.raises(ValueError):
        plan.poly_galois_keyswitch_prepared(a, -1, prepared, terms, w)
    with pytest.raises(eng.TinyNttError, match="overlap"):
        plan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w, out=a)                # in place is out of scope
    # out is checked like poly_gadget_multidot_prepared's: a host tensor or another word size never reaches the kernel
    with pytest.raises(eng.TinyNttError):
        plan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w, out=torch.empty((batch, 2, n), dtype=plan.torch_dtype))
    with pytest.raises(eng.TinyNttError):
        plan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w, out=torch.empty((batch, 2, n), dtype=torch.int32, device=a.device))
    with pytest.raises(ValueError):
        plan.poly_galois_keyswitch_prepared(a, g, prepared, terms, w, out=torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device))
    for bad in (0, -1):
        with pytest.raises(ValueError):
            plan.poly_galois_keyswitch_prepared(a, g, prepared, bad, w)
    torch.cuda.synchronize()
    assert torch.equal(c, last)
