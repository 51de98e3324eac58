"""Moduli at the boundaries of the arithmetic policies, shared by tests/test_policy_moduli_emu.py (CPU stepping) and
tests/test_gpu_policy_moduli.py (the kernels).  The library promises every entry point for any odd prime q < 2^62 = 1 (mod 2n):
the lazy policy where plan_tables.h's h_lazy_ok, h_pw_fast_ok and h_split_sched_ok allow it, the canonical policy otherwise, and
the base-case product at n = 4096 where h_bc_sched_ok passes.  The bound schedules behind those functions are tightest at the last
q = 2^k - c they accept, so this table holds, per size and word length, that prime and the next NTT prime below it (which they
refuse), the word-size points of the modulus sweeps (the largest NTT prime below 2^k and below 0.71 * 2^k for k = 20, 31, 32, 33, 41, 47,
61, 62), the largest NTT primes below 2^23 and 2^28 where they are not lazy, and the reference's moduli.

The numbers are literals: finding a boundary means visiting NTT primes, which is too slow for a test.  They were printed by
tools/find_policy_moduli.py, and tests/test_policy_moduli_emu.py::test_table_flags_and_boundary_pairs checks every flag and
every pair (one prime step each), so a change to a bound schedule that moves a boundary fails there and names the pair.

CG_PAIRS, CIN_PAIRS, MID_PAIRS and FLAG_ENTRIES cover the replays that PAIRS does not.  HostTables carries five flags: lazy, cg_lazy
(h_cg_lazy_ok), cg_sched (h_cg_sched_ok: the constant-geometry kernels with the static fold schedule, run at n = 4096), cin
(h_split_sched_cin_ok: the n = 4096 product kernel for promised-canonical inputs) and bc.  CG_PAIRS and CIN_PAIRS hold, for n = 4096,
the boundary pairs of cg_sched and cin where they are not the lazy policy's own pair: cg_sched at k = 59 and 60, cin at k = 60.  No pair
is committed for a flag that has no boundary of its own: cg_lazy equals lazy wherever the lanes are 64 bits wide, cg_sched and cin end
with lazy at k = 50 and 55, and all three are off with 32-bit lanes (k = 23, 26, 28); the self-check asserts exactly that at the
committed lazy pairs.  MID_PAIRS holds the lazy pairs of n = 512, 1024 and 2048 at k = 26 and 60.  FLAG_ENTRIES lists every prime of
those pairs, the n = 4096 lazy and bc pair primes at k = 59 and 60 and Q60 with all five flags: at n = 4096 / k = 60 the nested regions
all flags, no cin, no cin or cg_sched, lazy only, none; at k = 59 all flags, no cg_sched, no cg_sched or bc, none (cin ends with lazy
there).  Printed by tools/find_policy_moduli.py --tables flags (bisection and --walk agree), re-derived from tests/emu's
emu_plan_flags by tests/test_policy_flags_emu.py::test_flag_tables_and_boundary_pairs, stepped on the CPU by the rest of that file
and run on the GPU by tests/test_gpu_policy_flags.py (all but the cin kernel itself: the library is built without it, TN_FUSED_CIN = 0,
so only the CPU stepping and the replay guard that instantiation)."""
from chosen_rows import Q23, Q60, psi_of          # noqa: F401  (psi_of: psi of a plan of this table, for its users)

# (n, flag, last prime = 1 (mod 2n) with the flag walking down from 2^k, first without it)
PAIRS = [
    (256, "lazy", 8372737, 8365057),
    (256, "lazy", 66097153, 66091009),
    (256, "lazy", 1125899906720257, 1125899906701313),
    (256, "lazy", 36028797014771201, 36028797014768641),
    (256, "lazy", 576460752236319233, 576460752236305921),
    (256, "lazy", 1152921504571058177, 1152921504571045889),
    (4096, "lazy", 8380417, 8273921),
    (4096, "lazy", 66134017, 66052097),
    (4096, "lazy", 1125899906826241, 1125899906629633),
    (4096, "bc", 1125899906826241, 1125899906629633),
    (4096, "lazy", 36028797014876161, 36028797014704129),
    (4096, "bc", 36028797014876161, 36028797014704129),
    (4096, "lazy", 576460752236388353, 576460752236290049),
    (4096, "bc", 576460752241082369, 576460752241033217),
    (4096, "lazy", 1152921504571146241, 1152921504570802177),
    (4096, "bc", 1152921504577118209, 1152921504576864257),
    (8192, "lazy", 66404353, 66011137),
    (8192, "lazy", 1125899906826241, 1125899906629633),
    (8192, "lazy", 36028797015212033, 36028797014704129),
    (8192, "lazy", 576460752236412929, 576460752234823681),
    (8192, "lazy", 1152921504571146241, 1152921504570802177),
]
# (n, q, lazy, bc)
ENTRIES = [
    (256, 742913, False, False),
    (256, 1047041, False, False),
    (256, 8365057, False, False),
    (256, 8372737, True, False),
    (256, 8380417, True, False),
    (256, 66091009, False, False),
    (256, 66097153, True, False),
    (256, 268432897, False, False),
    (256, 1524706817, False, False),
    (256, 2147483137, False, False),
    (256, 3049426433, False, False),
    (256, 4294962689, False, False),
    (256, 6098851841, False, False),
    (256, 8589921281, False, False),
    (256, 1561306510849, False, False),
    (256, 2199023254529, False, False),
    (256, 99923616724993, False, False),
    (256, 140737488349697, True, False),
    (256, 1125899906701313, False, False),
    (256, 1125899906720257, True, False),
    (256, 36028797014768641, False, False),
    (256, 36028797014771201, True, False),
    (256, 576460752236305921, False, False),
    (256, 576460752236319233, True, False),
    (256, 1152921504571045889, False, False),
    (256, 1152921504571058177, True, False),
    (256, 1637148536541710849, False, False),
    (256, 2305843009213687297, False, False),
    (256, 3274297073083422721, False, False),
    (256, 4611686018427379201, False, False),
    (4096, 737281, False, False),
    (4096, 1032193, False, False),
    (4096, 8273921, False, False),
    (4096, 8380417, True, False),
    (4096, 66052097, False, False),
    (4096, 66134017, True, False),
    (4096, 268369921, False, False),
    (4096, 1524523009, False, False),
    (4096, 2147377153, False, False),
    (4096, 3049381889, False, False),
    (4096, 4294828033, False, False),
    (4096, 6098747393, False, False),
    (4096, 8589852673, False, False),
    (4096, 1561306423297, False, False),
    (4096, 2199023190017, False, False),
    (4096, 99923616710657, False, False),
    (4096, 140737488273409, False, False),
    (4096, 1125899906629633, False, False),
    (4096, 1125899906826241, True, True),
    (4096, 36028797014704129, False, False),
    (4096, 36028797014876161, True, True),
    (4096, 576460752236290049, False, False),
    (4096, 576460752236388353, True, False),
    (4096, 576460752241033217, True, False),
    (4096, 576460752241082369, True, True),
    (4096, 1152921504570802177, False, False),
    (4096, 1152921504571146241, True, False),
    (4096, 1152921504576864257, True, False),
    (4096, 1152921504577118209, True, True),
    (4096, 1152921504606830593, True, True),
    (4096, 1637148536541577217, False, False),
    (4096, 2305843009213554689, False, False),
    (4096, 3274297073082474497, False, False),
    (4096, 4611686018427322369, False, False),
    (8192, 737281, False, False),
    (8192, 1032193, False, False),
    (8192, 8273921, False, False),
    (8192, 66011137, False, False),
    (8192, 66404353, True, False),
    (8192, 268369921, False, False),
    (8192, 1524121601, False, False),
    (8192, 2147352577, False, False),
    (8192, 3049357313, False, False),
    (8192, 4294475777, False, False),
    (8192, 6098747393, False, False),
    (8192, 8589852673, False, False),
    (8192, 1561306398721, False, False),
    (8192, 2199023190017, False, False),
    (8192, 99923616710657, False, False),
    (8192, 140737488273409, False, False),
    (8192, 1125899906629633, False, False),
    (8192, 1125899906826241, True, False),
    (8192, 36028797014704129, False, False),
    (8192, 36028797015212033, True, False),
    (8192, 576460752234823681, False, False),
    (8192, 576460752236412929, True, False),
    (8192, 1152921504570802177, False, False),
    (8192, 1152921504571146241, True, False),
    (8192, 1152921504606830593, True, False),
    (8192, 1637148536541577217, False, False),
    (8192, 2305843009213317121, False, False),
    (8192, 3274297073082089473, False, False),
    (8192, 4611686018427322369, False, False),
]

# ---- the other replays of plan_tables.h: cg_sched (h_cg_sched_ok), cin (h_split_sched_cin_ok), and n = 512 / 1024 / 2048 ----
# Same shape as PAIRS.  Only boundaries that are not the lazy policy's own are listed (docstring above).
CG_PAIRS = [
    (4096, "cg_sched", 576460752241991681, 576460752241360897),
    (4096, "cg_sched", 1152921504583507969, 1152921504583262209),
]
CIN_PAIRS = [
    (4096, "cin", 1152921504603676673, 1152921504603381761),
]
MID_PAIRS = [
    (512, "lazy", 66097153, 66091009),
    (512, "lazy", 1152921504571058177, 1152921504571045889),
    (1024, "lazy", 66097153, 66091009),
    (1024, "lazy", 1152921504571058177, 1152921504571045889),
    (2048, "lazy", 66097153, 66052097),
    (2048, "lazy", 1152921504571146241, 1152921504571035649),
]
# (n, q, lazy, cg_lazy, cg_sched, cin, bc)
FLAG_ENTRIES = [
    (512, 66091009, False, False, False, False, False),
    (512, 66097153, True, False, False, False, False),
    (512, 1152921504571045889, False, False, False, False, False),
    (512, 1152921504571058177, True, True, False, False, False),
    (1024, 66091009, False, False, False, False, False),
    (1024, 66097153, True, False, False, False, False),
    (1024, 1152921504571045889, False, False, False, False, False),
    (1024, 1152921504571058177, True, True, False, False, False),
    (2048, 66052097, False, False, False, False, False),
    (2048, 66097153, True, False, False, False, False),
    (2048, 1152921504571035649, False, False, False, False, False),
    (2048, 1152921504571146241, True, True, False, False, False),
    (4096, 576460752236290049, False, False, False, False, False),
    (4096, 576460752236388353, True, True, False, True, False),
    (4096, 576460752241033217, True, True, False, True, False),
    (4096, 576460752241082369, True, True, False, True, True),
    (4096, 576460752241360897, True, True, False, True, True),
    (4096, 576460752241991681, True, True, True, True, True),
    (4096, 1152921504570802177, False, False, False, False, False),
    (4096, 1152921504571146241, True, True, False, False, False),
    (4096, 1152921504576864257, True, True, False, False, False),
    (4096, 1152921504577118209, True, True, False, False, True),
    (4096, 1152921504583262209, True, True, False, False, True),
    (4096, 1152921504583507969, True, True, True, False, True),
    (4096, 1152921504603381761, True, True, True, False, True),
    (4096, 1152921504603676673, True, True, True, True, True),
    (4096, 1152921504606830593, True, True, True, True, True),
]
FLAG_NAMES = ("lazy", "cg_lazy", "cg_sched", "cin", "bc")      # columns 2.. of FLAG_ENTRIES = bits 0.. of tests/emu's emu_plan_flags

WORD_K = (20, 31, 32, 33, 41, 47, 61, 62)          # word lengths of the word-size points (two entries per n and k)


def lane_bits(q):
    return 32 if q < 2 ** 31 else 64


def sum_terms(products, q):
    """Sum over axis 1 of canonical residues mod q, reduced after every term: 2q < 2^63 for every modulus of the contract, so no
    term count overflows the word (test_dot_emu.sum_mod adds first and needs terms * q < 2^64: five terms at 62 bits do not fit)."""
    import numpy as np
    acc = np.array(products[:, 0], dtype=np.uint64)
    for j in range(1, products.shape[1]):
        acc = (acc + products[:, j]) % np.uint64(q)
    return acc


def entry_id(e):
    return f"n{e[0]}_q{e[1]}"


def _quick():
    """The GPU test's subset: every boundary pair of n = 4096, the lazy pairs of n = 256 and n = 8192 at k = 26 and k = 60, the
    word-size points and the reference's moduli at n = 4096."""
    keep = {(n, q) for n, flag, first, second in PAIRS for q in (first, second)
            if n == 4096 or (flag == "lazy" and first.bit_length() in (26, 60))}
    return [e for e in ENTRIES if (e[0], e[1]) in keep or (e[0] == 4096 and (e[1].bit_length() in WORD_K or e[1] in (Q23, Q60)))]


QUICK = _quick()
BC_ENTRIES = [e for e in ENTRIES if e[3]]          # all at n = 4096, the only size with a base-case kernel
