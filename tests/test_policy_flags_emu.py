"""CPU stepping at the moduli of policy_moduli.FLAG_ENTRIES: the boundaries of the constant-geometry kernels' static fold schedule
(cg_sched), of the product kernel for promised-canonical inputs (cin) and of the lazy policy at n = 512, 1024 and 2048, beside the
n = 4096 lazy and base-case boundaries at 59 and 60 bits.  The table's flags are re-derived from plan_tables.h first
(emu_plan_flags); then the constant-geometry trips in every arithmetic a plan admits, the fused standalone transforms, the fused
cyclic product, inverse transforms of unreduced words and the promised-canonical-inputs product are compared with the oracle
(tests/flag_rows.py).  No GPU.  (GPU twin: tests/test_gpu_policy_flags.py.)"""
import ctypes

import numpy as np
import pytest

import test_policy_moduli_emu as policy_emu
from conftest import ntt_prime_below
from flag_rows import PLAIN, flag_rows
from policy_moduli import CG_PAIRS, CIN_PAIRS, ENTRIES, FLAG_ENTRIES, FLAG_NAMES, MID_PAIRS, PAIRS, Q60, entry_id, lane_bits, psi_of
from test_dot_emu import EmuDot
from test_gadget_emu import EmuGadget
from test_hat_emu import EmuHat
from test_prepared_emu import EmuPrepared

LAZY, CG_LAZY, CG_SCHED, CIN, BC = range(2, 7)             # columns of FLAG_ENTRIES
IDS = [entry_id(e) for e in FLAG_ENTRIES]
N4096 = [e for e in FLAG_ENTRIES if e[0] == 4096]
MID = [e for e in FLAG_ENTRIES if e[0] != 4096]
MID_RUNS = [(e, canonical) for e in MID for canonical in ((False, True) if e[LAZY] else (True,))]
CGA_SHOUP, CGA_SPLIT_CANON, CGA_SPLIT_LAZY, CGA_SPLIT_SCHED = range(4)          # cg_core.h's arithmetic modes (emu_cgm's am)


@pytest.fixture(scope="module")
def plan_flags(emu):
    emu.lib.emu_plan_flags.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]

    def get(n, q):
        m = emu.lib.emu_plan_flags(n, q, psi_of(n, q))
        assert 0 <= m < 2 ** len(FLAG_NAMES), (n, q, m)
        return tuple(bool(m >> i & 1) for i in range(len(FLAG_NAMES)))
    return get


@pytest.fixture(scope="module")
def prep():
    return EmuPrepared()


@pytest.fixture(scope="module")
def dot():
    return EmuDot()


@pytest.fixture(scope="module")
def hat():
    return EmuHat()


@pytest.fixture(scope="module")
def gadget():
    return EmuGadget()


flags = policy_emu.flags                                   # test_kernels_match_the_oracle's own fixture (emu_is_lazy, bc_enabled)


def test_flag_tables_and_boundary_pairs(plan_flags):
    """Every FLAG_ENTRIES literal is what h_build_tables decides (emu_plan_flags restates no bound), every new pair is two
    consecutive NTT primes, the first with the flag and the second without, and a flag without a pair of its own ends with the
    lazy policy.  A change to a replay that moves a boundary by one prime fails here and names the pair."""
    table = {(e[0], e[1]): e[2:] for e in FLAG_ENTRIES}
    assert len(table) == len(FLAG_ENTRIES)
    for (n, q), literal in table.items():
        assert (q - 1) % (2 * n) == 0 and q < 2 ** 62
        assert plan_flags(n, q) == literal, (n, q)
    old = {(n, q): (lazy, bc) for n, q, lazy, bc in ENTRIES}
    for key in set(table) & set(old):
        assert (table[key][0], table[key][4]) == old[key], key
    for n, flag, first, second in CG_PAIRS + CIN_PAIRS + MID_PAIRS:
        which = FLAG_NAMES.index(flag)
        assert ntt_prime_below(first, n) == second, (n, flag, first, second)
        assert first.bit_length() == second.bit_length()
        assert plan_flags(n, first)[which] and not plan_flags(n, second)[which], (n, flag, first, second)
        assert table[(n, first)][which] and not table[(n, second)][which], (n, flag, first, second)
    assert [(p[0], p[1], p[2].bit_length()) for p in CG_PAIRS] == [(4096, "cg_sched", 59), (4096, "cg_sched", 60)]
    assert [(p[0], p[1], p[2].bit_length()) for p in CIN_PAIRS] == [(4096, "cin", 60)]
    assert [(p[0], p[1], p[2].bit_length()) for p in MID_PAIRS] == [(n, "lazy", k) for n in (512, 1024, 2048) for k in (26, 60)]
    # a flag with no pair of its own: off with 32-bit lanes, and with 64-bit lanes it ends where lazy ends
    names = {"cg_lazy": 1, "cg_sched": 2, "cin": 3}
    own = {(flag, first.bit_length()) for _, flag, first, _ in CG_PAIRS + CIN_PAIRS}
    for n, flag, first, second in PAIRS + MID_PAIRS:
        if flag != "lazy":
            continue
        k = first.bit_length()
        for q in (first, second):
            got = plan_flags(n, q)
            if lane_bits(q) == 32:
                assert not (got[1] or got[2] or got[3]), (n, q)
                continue
            assert got[1] == got[0], ("cg_lazy", n, q)
            if n == 4096:
                for name in ("cg_sched", "cin"):
                    if (name, k) not in own:
                        assert got[names[name]] == got[0], (name, n, q)
    assert own == {("cg_sched", 59), ("cg_sched", 60), ("cin", 60)}


def test_flag_table_holds_every_region_and_both_sides_of_every_boundary():
    have = {(e[0], e[1]) for e in FLAG_ENTRIES}
    assert (4096, Q60) in have
    for n, flag, first, second in CG_PAIRS + CIN_PAIRS + MID_PAIRS + [p for p in PAIRS if p[0] == 4096 and p[2].bit_length() in (59, 60)]:
        assert {(n, first), (n, second)} <= have, (n, flag, first)
    regions = {k: {e[2:] for e in N4096 if e[1].bit_length() == k} for k in (59, 60)}
    #                    lazy   cg_lazy cg_sched cin    bc
    assert regions[60] == {(True, True, True, True, True), (True, True, True, False, True), (True, True, False, False, True),
                           (True, True, False, False, False), (False,) * 5}
    assert regions[59] == {(True, True, True, True, True), (True, True, False, True, True), (True, True, False, True, False),
                           (False,) * 5}
    for n in (512, 1024, 2048):
        for bits in (32, 64):
            assert {e[LAZY] for e in MID if e[0] == n and lane_bits(e[1]) == bits} == {True, False}, (n, bits)


@pytest.mark.parametrize("entry", FLAG_ENTRIES, ids=IDS)
def test_constant_geometry_trips_in_every_arithmetic(emu, oracle, entry):
    """cg_core.h's trips (emu.cgm): forward, inverse, product and twisted forward in each arithmetic the plan admits, and which
    ones it refuses: split records need a lazy plan with 64-bit lanes, per-butterfly lazy folds cg_lazy, the static fold schedule
    cg_sched.  Every GROUP x layout x twiddle source (wave-uniform trips from the global table or not; the product's inverse with and
    without the reversed table) on the plain rows and the unreduced inverse inputs; the chosen rows on one layout per GROUP."""
    n, q = entry[:2]
    psi = psi_of(n, q)
    fr = flag_rows(oracle, n, q)
    rows, extra = fr.a.shape[0], range(fr.a.shape[0], fr.x.shape[0])
    admitted = {CGA_SHOUP: True, CGA_SPLIT_CANON: entry[LAZY] and lane_bits(q) == 64, CGA_SPLIT_LAZY: entry[CG_LAZY],
                CGA_SPLIT_SCHED: entry[CG_SCHED]}
    if n == 4096 and lane_bits(q) == 64:
        assert admitted[CGA_SPLIT_CANON] == admitted[CGA_SPLIT_LAZY] == entry[LAZY]
    for gi, group in enumerate((1, 2, 4, 8)):
        for layout in (0, 1, 2):
            for am in range(4):
                at = (n, q, group, layout, am)
                kw = dict(group=group, layout=layout, am=am)
                if not admitted[am]:
                    for mode in range(4):
                        assert emu.cgm(n, q, psi, mode, fr.a[0], fr.b[0] if mode == 2 else None, **kw) is None, at
                    continue
                every = layout == (gi + am) % 3
                for r in range(rows if every else PLAIN):
                    for tw in (0, 1, 2, 3) if r < PLAIN else (0,):              # (the values do not depend on the twiddle source)
                        assert np.array_equal(emu.cgm(n, q, psi, 2, fr.a[r], fr.b[r], flags=tw, **kw), fr.prod[r]), (at, r, tw)
                        if tw < 2:
                            assert np.array_equal(emu.cgm(n, q, psi, 0, fr.a[r], flags=tw, **kw), fr.fwd[r]), (at, r, tw)
                            assert np.array_equal(emu.cgm(n, q, psi, 3, fr.a[r], flags=tw, **kw), fr.tfwd[r]), (at, r, tw)
                for r in list(range(rows if every else PLAIN)) + list(extra):
                    for tw in (0, 1) if r < PLAIN or r >= rows else (0,):
                        assert np.array_equal(emu.cgm(n, q, psi, 1, fr.x[r], flags=tw, **kw), fr.inv[r]), (at, r, tw)


@pytest.mark.parametrize("entry", FLAG_ENTRIES, ids=IDS)
def test_fused_transforms_product_and_cyclic_product(emu, oracle, entry):
    """The register-tiled standalone transforms (twist + forward, cg_ntt, cg_intt; the inverse also on unreduced words: a full-width
    row, q, 2q - 1, 2^k), the fused product and the fused cyclic product, under the policy the plan takes and forced canonical."""
    n, q = entry[:2]
    psi = psi_of(n, q)
    fr = flag_rows(oracle, n, q)
    assert emu.lib.emu_is_lazy(n, q, psi) == int(entry[LAZY])
    for canonical in (False, True):
        at = (n, q, canonical)
        got = emu.fused(n, q, psi, fr.a, fr.b, canonical=canonical)
        assert np.array_equal(got, fr.prod), (at, np.nonzero((got != fr.prod).any(axis=1))[0].tolist())
        got = emu.fused(n, q, psi, fr.a, fr.b, canonical=canonical, cyclic=True)
        assert np.array_equal(got, fr.cyc), (at, np.nonzero((got != fr.cyc).any(axis=1))[0].tolist())
        for r in range(fr.a.shape[0]):
            assert np.array_equal(emu.fused_ntt(n, q, psi, 0, fr.a[r], canonical), fr.tfwd[r]), (at, r)
            assert np.array_equal(emu.fused_ntt(n, q, psi, 1, fr.a[r], canonical), fr.fwd[r]), (at, r)
        for r in range(fr.x.shape[0]):
            assert np.array_equal(emu.fused_ntt(n, q, psi, 2, fr.x[r], canonical), fr.inv[r]), (at, r)


@pytest.mark.parametrize("entry", N4096, ids=[entry_id(e) for e in N4096])
def test_promised_canonical_inputs(emu, oracle, entry):
    """TN_PLAN_CANONICAL_INPUTS: the product kernel whose bound schedule starts from q is stepped exactly where cin holds (Q60, the
    last prime with it) and refused where it does not (the first prime without it, primes that are lazy without it, primes that are
    not lazy).  Rows in [0, q): the plain rows (all q - 1 among them) and the chosen-spectrum and boundary rows reduced mod q."""
    n, q = entry[:2]
    fr = flag_rows(oracle, n, q)
    assert int(fr.ra.max()) == q - 1 and (fr.ra[3] == q - 1).all()
    got = emu.fused(n, q, psi_of(n, q), fr.ra, fr.rb, promised_canonical_inputs=True)
    assert (got is None) == (not entry[CIN]), (n, q)
    if got is not None:
        assert np.array_equal(got, fr.prod), (n, q, np.nonzero((got != fr.prod).any(axis=1))[0].tolist())


def test_promised_canonical_inputs_visits_both_sides():
    cin = {(e[0], e[1]): e[CIN] for e in N4096}
    assert cin[(4096, Q60)] and not cin[(4096, 1152921504583507969)]                    # lazy and cg_sched without cin
    for n, _, first, second in CIN_PAIRS:
        assert cin[(n, first)] and not cin[(n, second)]
    assert any(e[LAZY] and not e[CIN] for e in N4096) and any(not e[LAZY] for e in N4096)


@pytest.mark.parametrize("entry,canonical", MID_RUNS, ids=[entry_id(e) + ("-canonical" if c else "-lazy") for e, c in MID_RUNS])
def test_mid_sizes_through_every_stepped_kernel(emu, prep, dot, hat, gadget, oracle, flags, entry, canonical):
    """n = 512, 1024 and 2048 at their lazy boundaries (26 and 60 bits): test_policy_moduli_emu.py's
    test_kernels_match_the_oracle, unchanged, on these entries (the fused product, prepared, dot-product, transform-domain and
    gadget kernels); the transforms and the cyclic product are in test_fused_transforms_product_and_cyclic_product."""
    assert not entry[BC]
    policy_emu.test_kernels_match_the_oracle(emu, prep, dot, hat, gadget, oracle, flags, (entry[0], entry[1], entry[LAZY], entry[BC]), canonical)
