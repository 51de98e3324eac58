"""The refusals of tn_poly_pack_step_prepared_dev and tn_lwe_embed_dev through the real library, in the style of
tests/test_gpu_api_cases.py: the status and the tn_last_error text of every fault of the two argument lists, on real buffers.  A call
that the library must refuse goes to the CPU stepping of the same checks first (tests/emu_pack: the list capi.cpp runs), so a
check that no longer refuses is found before a pointer of that call reaches the device; accepted calls run and are compared."""
import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from test_gpu_pack import explicit
from test_pack_emu import EmuPack

pytestmark = pytest.mark.gpu
FN, FNE = "tn_poly_pack_step_prepared_dev", "tn_lwe_embed_dev"


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def pack():
    return EmuPack()


@pytest.mark.parametrize("tag", ["P256", "P4096_60"])
def test_pack_step_refusals(eng, pack, tag):
    import torch
    n, q, psi = PARAMS[tag]
    k = q.bit_length()
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch, terms, w, g, rot = 5, 2, k // 2, 3, n // 2
    ev = plan.fill_lcg(batch * 2, 1, 2).reshape(batch, 2, n); od = plan.fill_lcg(batch * 2, 5, 2).reshape(batch, 2, n)
    prepared = plan.prepare(plan.fill_lcg(batch * 2 * terms, 2, 2))
    c = torch.empty((batch, 2, n), dtype=plan.torch_dtype, device=ev.device)
    stream = plan._stream_ptr(None)
    E, O, BH, C = ev.data_ptr(), od.data_ptr(), prepared.tensor.data_ptr(), c.data_ptr()
    row = n * plan.elem_bytes
    OK, EINVAL, EUNSUPPORTED = eng.TN_OK, eng.TN_EINVAL, eng.TN_EUNSUPPORTED
    view = (n, plan.elem_bytes, 1, 0, q)

    def call(e_, o_, rot_, g_, bh, sets, c_, batch_, terms_, w_=w, flags=0, want=EINVAL, text=None, p=plan, v=view):
        if want != OK:
            assert pack.check(v, e_, o_, rot_, g_, bh, c_, sets, batch_, terms_, w_, flags)[0] == want, (rot_, g_, text)
        st = lib.tn_poly_pack_step_prepared_dev(p._h if p is not None else None, e_, o_, rot_, g_, bh, sets, c_, batch_, terms_, w_, flags, stream)
        assert st == want, (st, lib.tn_last_error())
        if text is not None:
            assert lib.tn_last_error().decode() == FN + ": " + text

    call(E, O, rot, g, BH, batch, C, batch, terms, want=OK)
    call(E, None, 0, g, BH, batch, C, batch, terms, w, eng.GADGET_BALANCED, want=OK)                 # the trace step
    last = explicit(plan, ev, None, 0, g, prepared, terms, w, True)
    call(E, O, rot, g, BH, batch, C, batch, terms, p=None, v=(0, 0, 0, 0, 0), text="plan is NULL")
    for bad in (0, 4, 2 * n, 2 * n + 1, 2 ** 32 - 1):
        call(E, O, rot, bad, BH, batch, C, batch, terms, text=f"galois[0] = {bad} is not an odd element below 2n")
    for bad in (2 * n, 2 ** 32 - 1):
        call(E, O, bad, g, BH, batch, C, batch, terms, text=f"rot = {bad} is not below 2n")
    call(E, None, 1, g, BH, batch, C, batch, terms, text="rot must be 0 when od is NULL (the trace step)")
    call(E, O, rot, 4, BH, batch, C, batch, 0, text="galois[0] = 4 is not an odd element below 2n")         # the element before terms
    call(E, O, 2 * n, g, BH, batch, C, batch, 0, text=f"rot = {2 * n} is not below 2n")                      # the rotation before terms
    call(E, O, rot, g, BH, batch, C, batch, 0, text="terms must be at least 1")
    call(E, O, rot, g, BH, batch, C, batch, terms, w, 2, text="unknown flag bit")
    call(E, O, rot, g, BH, batch, C, batch, terms, 0, text="need 1 <= base_log and 2^base_log < q")
    call(E, O, rot, g, BH, batch, C, batch, terms, k, text="need 1 <= base_log and 2^base_log < q")
    call(E, O, rot, g, BH, batch, C, batch, 65, 1, text="(terms - 1) * base_log must be below 64")
    dummy = 4096
    for big_batch, big_terms in ((2 ** 30, 1), (2 ** 29, 2), (2 ** 63, 1)):
        call(dummy, dummy, rot, g, dummy, 1, dummy, big_batch, big_terms, 1, text="batch * 2 * terms too large for one call (max 2^31 - 1 digit rows)")
    call(None, None, 0, g, None, 1, None, 0, 3, want=OK)                                             # batch 0 launches nothing
    for e_, bh, c_ in ((None, BH, C), (E, None, C), (E, BH, None)):
        call(e_, O, rot, g, bh, batch, c_, batch, terms, text="NULL buffer")
    call(E, O, rot, g, BH, 2, C, batch, terms, text="bhat_sets must be 1 (one set of operands for every row) or batch")
    overlap = "output must not alias or overlap an input"
    for c_ in (E, O, BH, E + (batch * 2 - 1) * row, O - (batch * 2 - 1) * row, O + batch * 2 * row - 1):
        call(E, O, rot, g, BH, batch, c_, batch, terms, text=overlap)
    call(E, O, rot, g, BH, 1, BH + (2 * terms - 1) * row, batch, terms, text=overlap)                # a shared key's last row
    call(E, None, 0, g, BH, batch, E, batch, terms, text=overlap)                                    # the trace step does not run in place
    torch.cuda.synchronize()
    assert torch.equal(c, last)                                                                      # no refused call wrote to c

    # plans without the fused kernels refuse the call before they look at the element
    for other in (eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q))):
        assert not other.has_fused
        call(E, O, rot, 4, BH, batch, C, batch, terms, want=EUNSUPPORTED, p=other, v=(n, plan.elem_bytes, 0, 0, q),
             text="prepared operands need a plan with the fused kernels (tn_plan_has_fused)")

    # the Python side
    with pytest.raises(TypeError):
        plan.poly_pack_step_prepared(ev, plan.to_host(od), rot, g, prepared, terms, w)               # a device tensor and a host array
    with pytest.raises(ValueError):
        plan.poly_pack_step_prepared(ev, od[:3], rot, g, prepared, terms, w)                         # od of another batch
    with pytest.raises(ValueError):
        plan.poly_pack_step_prepared(ev.reshape(-1), od, rot, g, prepared, terms, w)
    with pytest.raises(ValueError):
        plan.poly_pack_step_prepared(ev, od, -1, g, prepared, terms, w)
    with pytest.raises(ValueError):
        plan.poly_pack_step_prepared(ev, od, rot, g, prepared, 0, w)
    with pytest.raises(eng.TinyNttError, match="overlap"):
        plan.poly_pack_step_prepared(ev, od, rot, g, prepared, terms, w, out=od)
    with pytest.raises(eng.TinyNttError, match="odd element below 2n"):
        plan.poly_pack_step_prepared(ev, od, rot, 2, prepared, terms, w)
    with pytest.raises(TypeError):
        plan.poly_pack_step_prepared(ev, od, rot, g, prepared.tensor, terms, w)
    torch.cuda.synchronize()
    assert torch.equal(c, last)


@pytest.mark.parametrize("tag", ["P256", "P4096_60"])
def test_embed_refusals_and_every_kind_of_plan(eng, pack, tag):
    import torch
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    lib = plan._lib
    batch = 3
    rng = np.random.default_rng(n)
    hl = rng.integers(0, 2 ** (8 * plan.elem_bytes) - 1, (batch, n + 1), dtype=np.uint64, endpoint=True)
    hl[0, :3] = (0, q, q - 1)
    lwe = torch.from_numpy(np.ascontiguousarray(hl.astype(plan.dtype)).view(np.int32 if plan.elem_bytes == 4 else np.int64)).to("cuda:0")
    want = {i: pack.embed(n, q, hl, i) for i in (0, 1, n - 1)}
    stream = plan._stream_ptr(None)
    view = (n, plan.elem_bytes, 1, 0, q)
    EINVAL = eng.TN_EINVAL
    for p in (plan, eng.get_general_plan(n, q, psi), eng.get_omega_plan(n, q, pow(psi, 2, q))):
        for index in want:
            buf = torch.full((batch * 2 + 2, n), 7, dtype=plan.torch_dtype, device="cuda:0")          # a guard row on either side
            a = p.lwe_embed(lwe, index, out=buf[1:-1].reshape(batch, 2, n))
            assert np.array_equal(plan.to_host(a).astype(np.uint64), want[index]), (tag, index)
            assert bool((buf[0] == 7).all()) and bool((buf[-1] == 7).all())
            back = p.sample_extract(a, index)
            assert np.array_equal(plan.to_host(back).astype(np.uint64), hl % np.uint64(q)), (tag, index)
    one = plan.lwe_embed(hl[1], 1)                                                                   # a host row in, a host ciphertext out
    assert isinstance(one, np.ndarray) and one.shape == (2, n) and np.array_equal(one.astype(np.uint64), want[1][1])
    a = torch.empty((batch, 2, n), dtype=plan.torch_dtype, device="cuda:0")
    L, A = lwe.data_ptr(), a.data_ptr()

    def call(l_, a_, batch_, index, text, h=plan._h, v=view):
        assert pack.check_embed(v, l_, a_, batch_, index)[0] == EINVAL, text
        assert lib.tn_lwe_embed_dev(h, l_, a_, batch_, index, stream) == EINVAL
        assert lib.tn_last_error().decode() == FNE + ": " + text

    call(L, A, batch, 0, "plan is NULL", None, (0, 0, 0, 0, 0))
    call(L, A, batch, n, "index must be below n")
    call(4096, 4096, 2 ** 31 // (n + 1) + 1, 0, "batch * (n + 1) too large for one call (max 2^31 - 1 words)")
    call(None, A, batch, 0, "NULL buffer")
    call(L, None, batch, 0, "NULL buffer")
    call(L, L, batch, 0, "output must not alias or overlap the input")
    call(L, L + batch * (n + 1) * plan.elem_bytes - 1, batch, 0, "output must not alias or overlap the input")
    assert lib.tn_lwe_embed_dev(plan._h, None, None, 0, 0, stream) == eng.TN_OK                       # batch 0 launches nothing
    with pytest.raises(ValueError):
        plan.lwe_embed(lwe[:, :n].contiguous())
    with pytest.raises(eng.TinyNttError, match="index must be below n"):
        plan.lwe_embed(lwe, n)
    torch.cuda.synchronize()
