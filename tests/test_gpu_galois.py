"""GPU tests of tn_automorphism_dev and tn_automorphism_prepared_dev (Plan.automorphism, Plan.automorphism_prepared): the ring
automorphisms a(x) -> a(x^g) on coefficient rows of every kind of plan and on prepared rows of fused plans, exact equality with
sigma_g written from its definition (tests/test_galois_emu.py: sigma), and the uses they are for."""

import ctypes

import numpy as np
import pytest

from conftest import PARAMS
from test_galois_emu import coefficient_rows, seeded_elements, sigma
from test_prepared_emu import shape_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


def make_plan(eng, kind):
    if kind == "general":                                     # nothing validated: an even modulus, any psi
        return eng.get_general_plan(64, 1000000, 3)
    if kind == "omega":
        return eng.get_omega_plan(32, 7681, 3)
    n, q, psi = shape_params(kind)
    return eng.get_plan(n, q, psi)


def elements(n):
    return [1, 3, n + 1, 2 * n - 1] + seeded_elements(n, 2, 17 * n)


def host(plan, t):
    return plan.to_host(t.reshape(-1, plan.n)).astype(np.uint64).reshape(tuple(t.shape))


@pytest.mark.parametrize("kind", ["P4", "general", "omega", "P256", "P1024", "P4096_60", "P8192_60"])
def test_coefficient_form_on_every_kind_of_plan(eng, kind):
    """Unreduced words, a row of zeros and a row of words = 0 mod q; batches 1 and 3 (and, at n = 256, 1,037 rows: 259 tiles
    of four rows and a last tile of one row); each element alone and four in one call."""
    plan = make_plan(eng, kind)
    n, q = plan.n, plan.q
    assert plan.has_fused == (kind in ("P256", "P1024", "P4096_60", "P8192_60"))
    gs = elements(n)
    for batch in (1, 3) + ((1037,) if kind == "P256" else ()):
        a = coefficient_rows(n, q, batch, n + batch)
        da = plan.to_device(a) if plan.elem_bytes == 8 else plan.to_device(a.astype(np.uint32))     # bit patterns, not values
        ref = {g: sigma(a, g, q) for g in gs}
        for g in gs:
            got = plan.automorphism(da, g)
            assert tuple(got.shape) == (batch, n)
            assert np.array_equal(host(plan, got), ref[g]), (kind, batch, g)
        for lst in (gs[:4], [gs[4], gs[1], gs[5], gs[1]]):
            got = plan.automorphism(da, lst)
            assert tuple(got.shape) == (batch, 4, n)
            hg = host(plan, got)
            for m, g in enumerate(lst):
                assert np.array_equal(hg[:, m], ref[g]), (kind, batch, lst, m)
        assert np.array_equal(host(plan, da), a)                                                     # the input is left alone
    if kind == "P256":
        # more tiles than workgroups stay resident (8 per CU): every workgroup goes round its tile loop more than once, the
        # last tile holds one row
        import torch
        batch = 2 * 4 * 8 * torch.cuda.get_device_properties(0).multi_processor_count + 5
        a = coefficient_rows(n, q, batch, 99)
        da = plan.to_device(a.astype(np.uint32))
        lst = [gs[4], gs[3], gs[5], gs[1]]
        hg = host(plan, plan.automorphism(da, lst))
        for m, g in enumerate(lst):
            assert np.array_equal(hg[:, m], sigma(a, g, q)), (kind, batch, m)
        xhat = plan.prepare(da)
        images = plan.automorphism_prepared(xhat, [gs[4], gs[1]]).tensor.reshape(batch, 2, n)
        for m, g in enumerate((gs[4], gs[1])):
            assert torch.equal(images[:, m].contiguous(), plan.prepare(sigma(a, g, q)).tensor), (kind, batch, m)


def test_host_values_and_shapes(eng):
    """Host arrays go in as values (negative ones taken mod q) and come back as host arrays; an int gives (batch, n), a
    sequence (batch, count, n); one polynomial gives (n,) and (count, n)."""
    n, q, psi = PARAMS["P256"]
    plan = eng.get_plan(n, q, psi)
    rng = np.random.default_rng(3)
    a = rng.integers(-q, q, (3, n), dtype=np.int64)
    ref = sigma((a % q).astype(np.uint64), 5, q)
    got = plan.automorphism(a, 5)
    assert isinstance(got, np.ndarray) and got.shape == (3, n) and np.array_equal(got, ref)
    got = plan.automorphism(a, [5, 2 * n - 1])
    assert got.shape == (3, 2, n) and np.array_equal(got[:, 0], ref) and np.array_equal(got[:, 1], sigma((a % q).astype(np.uint64), 2 * n - 1, q))
    one = plan.automorphism(a[1], 5)
    assert one.shape == (n,) and np.array_equal(one, ref[1])
    assert plan.automorphism(a[1], [5]).shape == (1, n)


HAT_PLANS = ["P256", "P1024", "P4096", "P4096_60", "P4096_60-canonical", "P8192_60"]


@pytest.mark.parametrize("kind", HAT_PLANS)
def test_prepared_form(eng, kind):
    """unprepare(automorphism_prepared(prepare(x), g)) == sigma_g(x) and automorphism_prepared(prepare(x), g) ==
    prepare(sigma_g(x)) word for word; three elements in one call equal three single calls.  P4096_60 as created holds
    prepared rows in the base-case format, under the canonical policy the complete transform."""
    import torch
    tag, canonical = kind.partition("-canonical")[0], kind.endswith("-canonical")
    n, q, psi = shape_params(tag)
    plan = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL if canonical else 0)
    x = coefficient_rows(n, q, 3, n)
    x[1] = 0; x[1, 1] = 1                                     # x^1
    xhat = plan.prepare(plan.to_device(x) if plan.elem_bytes == 8 else plan.to_device(x.astype(np.uint32)))
    before = xhat.tensor.clone()
    gs = elements(n)
    singles = {}
    for g in gs:
        want = sigma(x, g, q)
        got = plan.automorphism_prepared(xhat, g)
        assert isinstance(got, eng.PreparedOperand) and got.plan is plan and got.rows == 3
        singles[g] = got.tensor
        assert torch.equal(got.tensor, plan.prepare(want).tensor), (kind, g)
        assert np.array_equal(host(plan, plan.unprepare(got)), want), (kind, g)
    lst = [gs[1], gs[4], gs[1]]
    got = plan.automorphism_prepared(xhat, lst)
    assert got.rows == 9
    images = got.tensor.reshape(3, 3, n)
    for m, g in enumerate(lst):
        assert torch.equal(images[:, m], singles[g]), (kind, m)
    assert torch.equal(xhat.tensor, before)


@pytest.mark.parametrize("tag", ["P4096_60", "P1024"])
def test_hoisted_rotation_of_a_dot_product(eng, tag):
    """The use it is for, two terms: sum_j sigma_g(a_j) b_j == sigma_g(sum_j a_j sigma_{g^-1}(b_j)), the right side's sigma_g
    taken on coefficients (numpy) and on the prepared sum (automorphism_prepared, then unprepare)."""
    n, q, psi = PARAMS[tag]
    plan = eng.get_plan(n, q, psi)
    rng = np.random.default_rng(n)
    batch, terms = 3, 2
    a = rng.integers(0, q, (batch * terms, n), dtype=np.uint64)
    b = rng.integers(0, q, (batch * terms, n), dtype=np.uint64)
    for g in (3, seeded_elements(n, 1, 29)[0]):
        ginv = pow(g, -1, 2 * n)
        left = host(plan, plan.poly_dot_hat(plan.prepare(sigma(a, g, q)), plan.prepare(b), terms))
        ahat, bback = plan.prepare(a), plan.prepare(sigma(b, ginv, q))
        inner = host(plan, plan.poly_dot_hat(ahat, bback, terms))
        assert np.array_equal(left, sigma(inner, g, q)), (tag, g)
        kept = plan.poly_dot_hat(ahat, bback, terms, keep_prepared=True)
        assert np.array_equal(left, host(plan, plan.unprepare(plan.automorphism_prepared(kept, g)))), (tag, g)


def test_rotation_then_key_switch(eng):
    """poly_gadget_multidot_prepared on the device's sigma_g(a) equals the same call on the numpy sigma_g(a)."""
    import torch
    n, q, psi = PARAMS["P4096_60"]
    plan = eng.get_plan(n, q, psi)
    batch, outs, terms, w = 3, 2, 2, 30
    a = plan.fill_lcg(batch, 1, 2)
    key = plan.prepare(plan.fill_lcg(outs * terms, 9, 2))
    g = 5
    rotated = plan.automorphism(a, g)
    want = plan.to_device(sigma(host(plan, a), g, q))
    assert torch.equal(rotated, want)
    c = plan.poly_gadget_multidot_prepared(rotated, key, outs, terms, w, True)
    assert torch.equal(c, plan.poly_gadget_multidot_prepared(want, key, outs, terms, w, True))


def test_error_paths(eng):
    """Status and text on the device, one representative fault per step of the list, in its order."""
    import torch
    n, q, psi = PARAMS["P256"]
    plan = eng.get_plan(n, q, psi)
    general = eng.get_general_plan(n, q, psi)
    lib = plan._lib
    batch = 4
    a = plan.fill_lcg(batch, 1, 2)
    xhat = plan.prepare(a)
    out = torch.zeros((batch, 3, n), dtype=plan.torch_dtype, device=a.device)
    stream = plan._stream_ptr(None)
    A, X, C = a.data_ptr(), xhat.tensor.data_ptr(), out.data_ptr()
    row = n * plan.elem_bytes
    OK, EINVAL, EUNSUPPORTED = eng.TN_OK, eng.TN_EINVAL, eng.TN_EUNSUPPORTED

    def arr(*v):
        return (ctypes.c_uint32 * len(v))(*v)

    for fn, name, src in ((lib.tn_automorphism_dev, "tn_automorphism_dev", A), (lib.tn_automorphism_prepared_dev, "tn_automorphism_prepared_dev", X)):
        def expect(status, text, *args):
            assert fn(*args, stream) == status
            if text is not None:
                assert lib.tn_last_error().decode() == name + ": " + text
        expect(OK, None, plan._h, src, C, batch, arr(3, 5, 7), 3)
        expect(EINVAL, "plan is NULL", None, src, C, batch, arr(3), 1)
        expect(EINVAL, "count must be between 1 and TN_GALOIS_MAX (16)", plan._h, src, C, batch, arr(3), 0)
        expect(EINVAL, "count must be between 1 and TN_GALOIS_MAX (16)", plan._h, src, C, batch, arr(*[1] * 17), 17)
        expect(EINVAL, "galois[1] = 6 is not an odd element below 2n", plan._h, src, C, batch, arr(3, 6), 2)
        expect(EINVAL, f"galois[0] = {2 * n + 1} is not an odd element below 2n", plan._h, src, C, batch, arr(2 * n + 1), 1)
        expect(EINVAL, "batch * count too large for one call (max 2^31 - 1 output rows)", plan._h, 4096, 4096, 2 ** 29, arr(1, 3, 5, 7), 4)
        expect(OK, None, plan._h, None, None, 0, None, 3)                      # batch 0 launches nothing
        expect(EINVAL, "NULL buffer", plan._h, None, C, batch, arr(3), 1)
        expect(EINVAL, "NULL buffer", plan._h, src, C, batch, None, 1)
        expect(EINVAL, "output must not alias or overlap the input", plan._h, src, src, batch, arr(3), 1)
        expect(EINVAL, "output must not alias or overlap the input", plan._h, src, src + (batch - 1) * row, batch, arr(3, 5), 2)
    assert lib.tn_automorphism_dev(general._h, A, C, batch, arr(3), 1, stream) == OK                    # needs n and q alone
    assert lib.tn_automorphism_prepared_dev(general._h, X, C, batch, arr(3), 1, stream) == EUNSUPPORTED
    assert lib.tn_last_error().decode() == "tn_automorphism_prepared_dev: prepared operands need a plan with the fused kernels (tn_plan_has_fused)"

    # the Python side
    with pytest.raises(eng.TinyNttError, match="another plan"):
        eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL).automorphism_prepared(xhat, 3)
    with pytest.raises(TypeError):
        plan.automorphism_prepared(a, 3)
    # a PreparedOperand given as out is this plan's and holds rows * count rows; one of the right kind is written and handed back
    other = eng.get_plan(n, q, psi, 0, eng.PLAN_FORCE_CANONICAL)
    with pytest.raises(eng.TinyNttError, match="another plan"):
        plan.automorphism_prepared(xhat, 3, out=other.prepare(a))
    with pytest.raises(ValueError):
        plan.automorphism_prepared(xhat, [3, 5], out=plan.prepare(a))
    with pytest.raises(ValueError):
        plan.automorphism(a, 3, out=torch.empty((n, batch), dtype=plan.torch_dtype, device=a.device))
    dst = plan.prepare(a)
    got = plan.automorphism_prepared(xhat, 3, out=dst)
    assert got.tensor.data_ptr() == dst.tensor.data_ptr() and torch.equal(got.tensor, plan.automorphism_prepared(xhat, 3).tensor)
    with pytest.raises(eng.TinyNttError, match="galois\\[0\\] = 4"):
        plan.automorphism(a, 4)
    with pytest.raises(eng.TinyNttError, match="count must be"):
        plan.automorphism(a, [])
    with pytest.raises(ValueError):
        plan.automorphism(a, -3)
    with pytest.raises(ValueError):
        plan.automorphism(a, [3, 5], out=torch.empty((batch, n), dtype=plan.torch_dtype, device=a.device))
    torch.cuda.synchronize()
