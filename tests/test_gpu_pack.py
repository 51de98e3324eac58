"""GPU tests of tn_poly_pack_step_prepared_dev (Plan.poly_pack_step_prepared): one level of the LWE -> RLWE packing tree, or one
trace step, from one launch, bit for bit against the explicit route on the device (tn_monomial_mul_dev on od, the sum and the
difference mod q in torch, tn_poly_galois_keyswitch_prepared_dev on the difference, the addition of the sum) and against the CPU
stepping of the kernel (tests/emu_pack/emu_pack.cpp)."""

import numpy as np
import pytest

from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from test_gadget_emu import MODES, gadget_pairs
from test_galoisks_emu import key_rows
from test_pack_emu import BATCH, EmuPack, case_rows, elements, rotations
from test_prepared_emu import CASES, CASE_IDS, _case_data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def pack():
    return EmuPack()


def explicit(plan, ev, od, rot, g, prepared, terms, w, balanced):
    """The contract on the device: monomial_mul on od with the exponent rot (and on ev with the exponent 0: ev mod q, word for
    word); s and d mod q in 64-bit torch integers (canonical words, q < 2^62); poly_galois_keyswitch_prepared on d; s added."""
    import torch
    n, q = plan.n, plan.q
    batch = int(ev.shape[0])
    e = plan.monomial_mul(ev, np.zeros(batch, dtype=np.int64)).to(torch.int64)
    t = plan.monomial_mul(od, np.full(batch, rot, dtype=np.int64)).to(torch.int64) if od is not None else torch.zeros_like(e)
    s, d = e + t, e - t
    s = torch.where(s >= q, s - q, s)
    d = torch.where(d < 0, d + q, d).to(plan.torch_dtype)
    c = plan.poly_galois_keyswitch_prepared(d, g, prepared, terms, w, balanced).to(torch.int64) + s
    return torch.where(c >= q, c - q, c).to(plan.torch_dtype)


def dev(plan, h):
    return plan.to_device(h.reshape(-1, plan.n)).reshape(h.shape)


def host(plan, c):
    return plan.to_host(c.reshape(-1, plan.n)).astype(np.uint64).reshape(tuple(c.shape))


def check_parity(eng, plan, pack, n, q, psi, a, b, canonical):
    """Batch 7, every (terms, w), a shared key and a key per row, both digit modes.  Below n = 4096 the whole element x rotation
    product against the route in every group; from n = 4096 on one seeded rotation per element.  The trace step for every element.
    The stepping is compared on one rotation per element and group, in turn, and on every trace step."""
    import torch
    assert plan.has_fused
    a, b = np.array(a), np.array(b)
    gs, rots = elements(n), rotations(n)
    turn = 0
    for first, (terms, w) in enumerate(gadget_pairs(q)):
        hev, hod = case_rows(a, b, first)
        ev, od = dev(plan, hev), dev(plan, hod)
        for shared in (True, False):
            idx = key_rows(BATCH, terms, shared)
            prepared = plan.prepare(b[idx[0].ravel()] if shared else b[idx.ravel()])
            bhat = plan.to_host(prepared.tensor).astype(np.uint64)
            for balanced in MODES:
                stepped = {(g, rots[(i + turn) % len(rots)]) for i, g in enumerate(gs)} if n < 4096 else {(g, rots[-1]) for g in gs}
                grid = [(g, r) for g in gs for r in rots] if n < 4096 else sorted(stepped)
                turn += 1
                for g, rot in grid:
                    where = (terms, w, shared, balanced, g, rot)
                    c = plan.poly_pack_step_prepared(ev, od, rot, g, prepared, terms, w, balanced)
                    assert c.shape == (BATCH, 2, n)
                    assert torch.equal(c, explicit(plan, ev, od, rot, g, prepared, terms, w, balanced)), where
                    if (g, rot) in stepped:
                        assert np.array_equal(host(plan, c), pack.step(n, q, psi, hev, hod, rot, g, bhat, terms, w, balanced, canonical)), where
                for g in gs:
                    c = plan.poly_pack_step_prepared(ev, None, 0, g, prepared, terms, w, balanced)
                    assert torch.equal(c, explicit(plan, ev, None, 0, g, prepared, terms, w, balanced)), (terms, w, shared, balanced, g, "trace")
                    assert np.array_equal(host(plan, c), pack.step(n, q, psi, hev, None, 0, g, bhat, terms, w, balanced, canonical)), (g, "trace")


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pack_step_equals_the_explicit_route_and_the_stepping(eng, pack, case):
    n, q, psi, a, b = _case_data(case)
    plan = eng.get_plan(n, q, psi)
    check_parity(eng, plan, pack, n, q, psi, a, b, False)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_pack_step_on_a_canonical_policy_plan(eng, pack, tag):
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    assert not plan.is_lazy
    check_parity(eng, plan, pack, n, q, psi, a, b, True)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_trace_step_is_ev_plus_its_homomorphic_automorphism(eng, tag):
    """od=None: c = ev + EvalAuto(ev, g), the automorphism key switch of ev mod q with ev mod q added; and it equals the pack form
    on an od of zeros, whatever the rotation.  Host arrays and one ciphertext go in and come out as in the other calls."""
    import torch
    n, q, psi, a, b = _case_data(tag)
    plan = eng.get_plan(n, q, psi)
    terms, w = gadget_pairs(q)[1]
    hev, _ = case_rows(np.array(a), np.array(b))
    ev = dev(plan, hev)
    prepared = plan.prepare(np.array(b)[key_rows(1, terms, True)[0].ravel()])
    e = plan.monomial_mul(ev, np.zeros(BATCH, dtype=np.int64))
    for g in elements(n):
        c = plan.poly_pack_step_prepared(ev, None, 0, g, prepared, terms, w, True)
        want = plan.poly_galois_keyswitch_prepared(e, g, prepared, terms, w, True).to(torch.int64) + e.to(torch.int64)
        assert torch.equal(c, torch.where(want >= q, want - q, want).to(plan.torch_dtype)), g
        assert torch.equal(c, plan.poly_pack_step_prepared(ev, torch.zeros_like(ev), n - 1, g, prepared, terms, w, True)), g
    ref = host(plan, c)
    hc = plan.poly_pack_step_prepared(hev, None, 0, g, prepared, terms, w, True)
    assert isinstance(hc, np.ndarray) and hc.shape == (BATCH, 2, n) and np.array_equal(hc, ref)
    one = plan.poly_pack_step_prepared(ev[2], None, 0, g, prepared, terms, w, True)
    assert one.shape == (2, n) and np.array_equal(plan.to_host(one), ref[2])
    with pytest.raises(eng.TinyNttError, match="rot must be 0"):
        plan.poly_pack_step_prepared(ev, None, 1, g, prepared, terms, w, True)


@pytest.mark.parametrize("fewer", [0, 1], ids=["dynamic", "one-row-fewer"])
def test_row_hand_out(eng, pack, fewer):
    """The smallest batch at n = 4096 / 60-bit, terms = 2 that plan_rows hands out through the device counter (the launcher plans
    an output row as the automorphism key switch does: dot_row_bytes, terms * n * 8 bytes), and one row fewer, which keeps the
    fixed stride; guard rows behind c stay as they were."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    terms, w, g, rot = 2, 30, 2 * n - 1, n // 2
    resident = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    rows = smallest_dynamic_batch(terms * n * plan.elem_bytes, resident) - fewer
    ev = plan.fill_lcg(rows * 2, 1, 2).reshape(rows, 2, n); od = plan.fill_lcg(rows * 2, 6, 2).reshape(rows, 2, n)
    b = plan.fill_lcg(rows * 2 * terms, 2, 2)
    per_set, shared = plan.prepare(b), plan.prepare(b[:2 * terms])
    before = ev.clone(), od.clone()
    buf = plan.fill_lcg(rows * 2 + 4, 9, 2)                         # c and two guard rows on either side
    guards = buf[:2].clone(), buf[-2:].clone()
    c = buf[2:-2].reshape(rows, 2, n)
    plan.poly_pack_step_prepared(ev, od, rot, g, per_set, terms, w, True, out=c)
    assert torch.equal(c, explicit(plan, ev, od, rot, g, per_set, terms, w, True))
    assert torch.equal(buf[:2], guards[0]) and torch.equal(buf[-2:], guards[1])
    c_shared = plan.poly_pack_step_prepared(ev, od, 1, 5, shared, terms, w, True)
    assert torch.equal(c_shared, explicit(plan, ev, od, 1, 5, shared, terms, w, True))
    c_trace = plan.poly_pack_step_prepared(ev, None, 0, 3, shared, terms, w, True)
    assert torch.equal(c_trace, explicit(plan, ev, None, 0, 3, shared, terms, w, True))
    assert torch.equal(ev, before[0]) and torch.equal(od, before[1])
    # a few rows, among them the first and last of the launch and of chunks in between, against the CPU stepping
    idx = sorted({0, 1, rows // 6 - 1, rows // 6, 1777 % rows, rows // 2 - 1, rows // 2, rows - 1})
    sel = torch.tensor(idx, device=ev.device)
    hb = plan.to_host(per_set.tensor.reshape(rows, 2 * terms, n)[sel].reshape(-1, n)).astype(np.uint64)
    assert np.array_equal(host(plan, c[sel]), pack.step(n, q, psi, host(plan, ev[sel]), host(plan, od[sel]), rot, g, hb, terms, w, True))


def test_guard_rows_behind_c_stay_untouched_at_a_small_batch(eng):
    """Batch 7 at n = 256 and n = 1024: two guard rows in front of and behind c keep their words, for the pack and the trace form."""
    import torch
    for tag in ("P256", "P1024"):
        n, q, psi = PARAMS[tag]
        plan = eng.get_plan(n, q, psi)
        terms, w = gadget_pairs(q)[0]
        ev = plan.fill_lcg(BATCH * 2, 1, 2).reshape(BATCH, 2, n); od = plan.fill_lcg(BATCH * 2, 3, 2).reshape(BATCH, 2, n)
        prepared = plan.prepare(plan.fill_lcg(2 * terms, 2, 2))
        for o, rot in ((od, 2 * n - 1), (None, 0)):
            buf = plan.fill_lcg(BATCH * 2 + 4, 9, 2)
            guards = buf[:2].clone(), buf[-2:].clone()
            c = buf[2:-2].reshape(BATCH, 2, n)
            plan.poly_pack_step_prepared(ev, o, rot, n + 1, prepared, terms, w, False, out=c)
            assert torch.equal(c, explicit(plan, ev, o, rot, n + 1, prepared, terms, w, False))
            assert torch.equal(buf[:2], guards[0]) and torch.equal(buf[-2:], guards[1]), (tag, rot)


def test_capture_into_a_graph_replays_the_captured_values_on_new_words(eng):
    """One launch captured into a graph (one kernel node, no parallel branches) and replayed twice onto a zeroed output, ev and od
    CHANGED in place between the replays: each replay equals a direct launch on the words that were in ev and od when it ran, with
    the rotation and the Galois element the launch was captured with (they travel by value)."""
    import torch
    n, q, psi = PARAMS["P1024"]
    plan = eng.get_plan(n, q, psi)
    terms, w = gadget_pairs(q)[0]
    rows, g, rot = 300, 5, n // 4
    prepared = plan.prepare(plan.fill_lcg(2 * terms, 4, 2))
    evs = [plan.fill_lcg(rows * 2, seed, 2).reshape(rows, 2, n) for seed in (3, 5, 7)]
    ods = [plan.fill_lcg(rows * 2, seed, 2).reshape(rows, 2, n) for seed in (11, 13, 17)]
    refs = [plan.poly_pack_step_prepared(x, y, rot, g, prepared, terms, w, True) for x, y in zip(evs, ods)]
    assert torch.equal(refs[0], explicit(plan, evs[0], ods[0], rot, g, prepared, terms, w, True)) and not torch.equal(refs[1], refs[2])
    ev, od = evs[0].clone(), ods[0].clone()
    s1 = torch.cuda.Stream(); c = torch.zeros_like(refs[0])
    torch.cuda.synchronize()          # the inputs, the references and the zero fill ran on the default stream: s1 starts behind them
    with torch.cuda.stream(s1):
        plan.poly_pack_step_prepared(ev, od, rot, g, prepared, terms, w, True, out=c, stream=s1)     # warm-up outside the capture
    s1.synchronize()
    assert torch.equal(c, refs[0])
    graph = torch.cuda.CUDAGraph(); c.zero_(); torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s1):
        plan.poly_pack_step_prepared(ev, od, rot, g, prepared, terms, w, True, out=c, stream=s1)
    for rep in (1, 2):
        c.zero_(); ev.copy_(evs[rep]); od.copy_(ods[rep]); torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(c, refs[rep]), rep
