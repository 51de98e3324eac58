"""GPU tests at the moduli of policy_moduli.FLAG_ENTRIES: the product, the three transforms and the cyclic product, through the
fused kernels and the constant-geometry kernels, on both sides of the cg_sched and cin boundaries and of the 59- and 60-bit lazy and
base-case boundaries of n = 4096 (so the scheduled, the per-butterfly lazy and the canonical constant-geometry kernels each meet a
59/60-bit boundary); inverse transforms of unreduced words; n = 512, 1024 and 2048 at their lazy boundaries; and that creating a
plan with PLAN_CANONICAL_INPUTS does no harm (the tested build does not contain the kernel instantiation for that promise, so
the device side of it is NOT covered here: see test_promise_of_canonical_inputs_is_harmless).  Every result is compared with the
oracle first (tests/flag_rows.py).  The CPU stepping of the same kernels is tests/test_policy_flags_emu.py; nothing here needs it
but launch_plan.h's plan_rows."""
import numpy as np
import pytest

import test_gpu_policy_moduli as gpu_policy
from emu_library import smallest_dynamic_batch
from flag_rows import flag_rows
from policy_moduli import CG_PAIRS, CIN_PAIRS, FLAG_ENTRIES, PAIRS, Q60, entry_id, psi_of
from test_gpu_parity import CG_SWEEP

pytestmark = pytest.mark.gpu

LAZY, CG_LAZY, CG_SCHED, CIN, BC = range(2, 7)             # columns of FLAG_ENTRIES
ENTRY = {(e[0], e[1]): e for e in FLAG_ENTRIES}
# both primes of the cg_sched and cin pairs: every constant-geometry variant
NEW = [ENTRY[(n, q)] for n, _, first, second in CG_PAIRS + CIN_PAIRS for q in (first, second)]
# the n = 4096 lazy and base-case pair primes at 59 and 60 bits (lazy or not, never cg_sched): one variant per LDS layout family
OLD = [ENTRY[(n, q)] for n, _, first, second in PAIRS if n == 4096 and first.bit_length() in (59, 60) for q in (first, second)]
OLD_VARIANTS = ["cg", "cg8", "cg8_swizzled"]
BOUNDARY = [(e, CG_SWEEP) for e in NEW] + [(e, OLD_VARIANTS) for e in OLD]
MID = [e for e in FLAG_ENTRIES if e[0] != 4096]
# Q60, both sides of the cin boundary, and a prime that is lazy (and cg_sched) without cin
CIN_CASES = [ENTRY[(4096, q)] for q in [Q60] + [q for p in CIN_PAIRS for q in p[2:]] + [1152921504583507969]]


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


def same(plan, got, want, at):
    """Device result against the oracle's rows; on a mismatch the message counts the differing coefficients."""
    h = plan.to_host(got).astype(np.uint64)
    assert np.array_equal(h, want), (at, f"{np.count_nonzero(h != want)} coefficients differ in rows {np.nonzero((h != want).any(axis=1))[0].tolist()}")


def check_transforms_and_products(plan, fr, variants, reduced=False):
    """poly_mult, ntt_forward, twisted_ntt_forward, cyclic_poly_mult on every operand row and ntt_inverse on those and the unreduced
    inverse inputs (reduced: all of them mod q first), per variant, against the oracle results computed once in fr."""
    Q = np.uint64(fr.q)
    da, db, dx = (plan.to_device(v % Q if reduced else np.array(v)) for v in (fr.a, fr.b, fr.x))      # (copies: fr's rows are read-only)
    for v in variants:
        at = (fr.n, fr.q, v)
        same(plan, plan.poly_mult(da, db, variant=v), fr.prod, at + ("poly_mult",))
        same(plan, plan.ntt_forward(da, variant=v), fr.fwd, at + ("ntt_forward",))
        same(plan, plan.ntt_inverse(dx, variant=v), fr.inv, at + ("ntt_inverse",))
        same(plan, plan.twisted_ntt_forward(da, variant=v), fr.tfwd, at + ("twisted_ntt_forward",))
        same(plan, plan.cyclic_poly_mult(da, db, variant=v), fr.cyc, at + ("cyclic_poly_mult",))


@pytest.mark.parametrize("entry,variants", BOUNDARY, ids=[entry_id(e) for e, _ in BOUNDARY])
def test_transforms_and_products_at_flag_boundaries(eng, oracle, entry, variants):
    n, q = entry[:2]
    psi = psi_of(n, q)
    plan = eng.Plan(n, q, psi)
    try:
        assert plan.has_fused and plan.is_lazy == entry[LAZY] and plan.elem_bytes == 8
        check_transforms_and_products(plan, flag_rows(oracle, n, q), ["fused"] + variants)
    finally:
        plan.close()


def test_boundary_cases_cover_every_constant_geometry_arithmetic(eng):
    """kernels.hip's launch_cg picks the slice of cg_part.hip from (lazy, cg_lazy, cg_sched): the cases above hold each of the
    three on 64-bit lanes at 59 and at 60 bits.  tn_kernel_name answers "cg_kernel" for every slice, so the name cannot tell the two
    sides of a cg_sched pair apart (asserted here so that a name that starts to tell them gets used); which slice runs rests on the
    flags, which tests/test_policy_flags_emu.py::test_flag_tables_and_boundary_pairs re-derives from plan_tables.h."""
    for k in (59, 60):
        kinds = {(e[LAZY], e[CG_LAZY], e[CG_SCHED]) for e, _ in BOUNDARY if e[1].bit_length() == k}
        assert kinds == {(True, True, True), (True, True, False), (False, False, False)}, k
    for n, _, first, second in CG_PAIRS:
        names = []
        for q in (first, second):
            plan = eng.Plan(n, q, psi_of(n, q))
            names.append([plan.kernel_name(v) for v in CG_SWEEP])
            plan.close()
        assert names[0] == names[1] == ["cg_kernel"] * len(CG_SWEEP)


@pytest.mark.parametrize("entry", CIN_CASES, ids=[entry_id(e) for e in CIN_CASES])
def test_promise_of_canonical_inputs_is_harmless(eng, oracle, entry):
    """What this can and cannot show.  The library under test is built with TN_FUSED_CIN = 0 (fused_kernels.h), so the product
    kernel's second instantiation, whose bound schedule starts from q, is NOT in it: a plan created with PLAN_CANONICAL_INPUTS
    accepts the promise and launches the same any-word kernel as the default plan, at every modulus, with or without cin
    (kernels.hip launch_fused_t).  No error in that instantiation's fold schedule could fail here; it is guarded by the replay
    h_split_sched_cin_ok and by the CPU stepping alone (test_policy_flags_emu.py::test_promised_canonical_inputs).  This test
    checks that the flag is harmless: such a plan is created at Q60, on both sides of the cin boundary and at a prime that is lazy
    without cin, and on rows in [0, q) (random, all q - 1, zero, x^(n-1) * x, the chosen-spectrum and boundary rows reduced mod q)
    its fused product, its other entry points and a constant-geometry variant equal the oracle.  The comparison with the default
    plan's product is bit for bit; in this build it compares a kernel with itself and would tell only if a build with
    TN_FUSED_CIN = 1 were put under the suite."""
    import torch
    n, q = entry[:2]
    psi = psi_of(n, q)
    fr = flag_rows(oracle, n, q)
    zero = np.zeros((1, n), dtype=np.uint64)
    a, b = np.concatenate([fr.ra, zero, fr.ra[:1]]), np.concatenate([fr.rb, fr.rb[:1], zero])
    want = np.concatenate([fr.prod, zero, zero])
    assert int(a.max()) == q - 1 and (a[3] == q - 1).all() and (b[3] == q - 1).all()
    default = eng.get_plan(n, q, psi)
    plan = eng.Plan(n, q, psi, 0, eng.PLAN_CANONICAL_INPUTS)
    try:
        assert plan.is_lazy and default.is_lazy and plan.has_fused
        assert plan.kernel_name("fused") == default.kernel_name("fused")
        da, db = plan.to_device(a), plan.to_device(b)
        c = plan.poly_mult(da, db, variant="fused")
        same(plan, c, want, (n, q, "canonical inputs"))
        assert torch.equal(c, default.poly_mult(da, db, variant="fused")), (n, q)
        check_transforms_and_products(plan, fr, ["fused", "cg8"], reduced=True)
    finally:
        plan.close()


def test_promise_of_canonical_inputs_with_rows_from_the_counter(eng, oracle):
    """The same plan (last prime with cin) on a ragged batch that plan_rows hands out through the device counter: one row more
    than the smallest dynamic batch with 4 workgroups per CU resident (emu_library.smallest_dynamic_batch, as the other
    test_dynamic_row_hand_out tests size theirs).  In the tested build this is the any-word kernel again (see above), so it adds
    to test_gpu_prepared.py::test_dynamic_row_hand_out only the modulus and the odd row count."""
    import torch
    n, q = CIN_PAIRS[0][0], CIN_PAIRS[0][2]
    psi = psi_of(n, q)
    default = eng.get_plan(n, q, psi)
    plan = eng.Plan(n, q, psi, 0, eng.PLAN_CANONICAL_INPUTS)
    try:
        least = smallest_dynamic_batch(n * plan.elem_bytes, 4 * torch.cuda.get_device_properties(0).multi_processor_count)
        rows = least + 1
        big_a, big_b = default.fill_lcg(rows, 1, 2), default.fill_lcg(rows, 2, 2)
        for t in (big_a, big_b):
            assert int(t.min()) >= 0 and int(t.max()) < q                 # (q < 2^63: the signed view compares like the words)
        c = plan.poly_mult(big_a, big_b, variant="fused")
        assert torch.equal(c, default.poly_mult(big_a, big_b, variant="fused")), (n, q, rows)
        sel = torch.tensor([0, 1, 511, 512, 1777, least - 1, least], device=c.device)
        same(plan, c[sel], oracle.poly_mult(plan.to_host(big_a[sel]).astype(np.uint64), plan.to_host(big_b[sel]).astype(np.uint64), q, psi),
             (n, q, rows))
    finally:
        plan.close()


@pytest.mark.parametrize("entry", MID, ids=[entry_id(e) for e in MID])
def test_mid_sizes_at_their_lazy_boundaries(eng, oracle, entry):
    """n = 512, 1024 and 2048: test_gpu_policy_moduli.py's check_entry (product, prepared, dot, transform-domain and gadget entry
    points), the fused standalone transforms and the fused cyclic product, on the plan the library picks and, for a lazy one, on the
    forced canonical plan too."""
    n, q = entry[:2]
    psi = psi_of(n, q)
    fr = flag_rows(oracle, n, q)
    for flags in ((0, eng.PLAN_FORCE_CANONICAL) if entry[LAZY] else (0,)):
        plan = eng.Plan(n, q, psi, 0, flags)
        try:
            assert plan.has_fused and plan.is_lazy == (entry[LAZY] and flags == 0), (n, q, flags)
            assert plan.elem_bytes == (4 if q < 2 ** 31 else 8)
            gpu_policy.check_entry(eng, plan, oracle, n, q, psi)
            check_transforms_and_products(plan, fr, ["fused"])
        finally:
            plan.close()
