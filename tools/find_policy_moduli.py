#!/usr/bin/env python3
"""One-off finder of the policy-boundary moduli committed as literals in tests/policy_moduli.py.  CPU only.

For n = 256, 4096 and 8192 (or --n ...) and every word length k of K_BOUNDARY it looks, among the NTT primes q = 1 (mod 2n)
below 2^k, for the boundary of the lazy policy (plan_tables.h: h_lazy_ok, h_pw_fast_ok and h_split_sched_ok, asked through
emu_is_lazy of tests/emu) and, at n = 4096, of the base case (h_bc_sched_ok, asked through bc_enabled): the pair of
consecutive NTT primes of which the upper still has the flag and the lower has not.  It then adds the word-size points of the
modulus sweeps (the largest NTT prime below 2^k and below 0.71 * 2^k for k of K_WORD) and the reference's moduli, asks the same
two functions for every entry's flags, and prints the body of tests/policy_moduli.py: PAIRS and ENTRIES.

By default a boundary is found by bisection over the primes between 2^(k-1) and 2^k, which takes seconds and assumes that a
flag which holds for the largest prime below 2^k holds for every prime down to the boundary: every bound the schedules check
grows with c = 2^k - q.  --walk visits every NTT prime from 2^k downwards instead and needs no such assumption (minutes per
pair at n = 256 for k = 59 and 60).  Both found the same pairs when the table was made.
tests/test_policy_moduli_emu.py::test_table_flags_and_boundary_pairs re-checks every literal in one prime step per pair.

--tables flags prints the tables of the other replays instead (--tables all, the default, prints both): for n = 4096 and every k
of K_BOUNDARY the boundaries of cg_lazy, cg_sched and cin (HostTables' flags, asked through emu_plan_flags) where they are not
the lazy pair itself, as CG_PAIRS and CIN_PAIRS; the lazy boundaries of n = 512, 1024 and 2048 at k = 26 and 60 as MID_PAIRS;
and FLAG_ENTRIES, all five flags of every prime of those pairs, of the n = 4096 lazy and bc pairs at k = 59 and 60 and of Q60.
cg_sched has pairs of its own at k = 59 and 60 and cin at k = 60; cg_lazy has none, nor have cg_sched and cin at k <= 55.
Bisection (3 s) and --walk (1 min) printed the same text when these tables were made, the cg_sched pairs at k = 59 and 60 and the
cin pair at k = 60 among it.  tests/test_policy_flags_emu.py::test_flag_tables_and_boundary_pairs re-checks every literal."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from conftest import Emu, is_prime, ntt_prime_below          # noqa: E402
from tiny_ntt_amd import numtheory                           # noqa: E402

K_BOUNDARY = (23, 26, 28, 50, 55, 59, 60)
K_WORD = (20, 31, 32, 33, 41, 47, 61, 62)
Q23, Q60 = 8380417, 1152921504606830593
REFERENCE = [(256, Q23), (4096, Q23), (4096, Q60), (8192, Q60)]


FLAG_NAMES = ("lazy", "cg_lazy", "cg_sched", "cin", "bc")          # bit order of emu_plan_flags (tests/emu/emu_kernels.cpp)
MID_N, MID_K = (512, 1024, 2048), (26, 60)
K_FLAGS = (59, 60)                                                  # word lengths whose n = 4096 lazy / bc pairs join FLAG_ENTRIES


class Flags:
    def __init__(self):
        import ctypes
        self.lib = Emu().lib
        self.lib.bc_enabled.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
        self.lib.emu_plan_flags.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
        self.cache, self.masks = {}, {}

    def mask(self, n, q):
        """(lazy, cg_lazy, cg_sched, cin, bc) of the plan (n, q): HostTables' own flags, through emu_plan_flags."""
        if (n, q) not in self.masks:
            m = self.lib.emu_plan_flags(n, q, numtheory.primitive_2n_root(n, q))
            assert 0 <= m < 32, (n, q, m)
            self.masks[(n, q)] = tuple(bool(m >> i & 1) for i in range(len(FLAG_NAMES)))
        return self.masks[(n, q)]

    def has(self, name):
        which = FLAG_NAMES.index(name)
        return lambda n, q: self.mask(n, q)[which]

    def __call__(self, n, q):
        """(lazy, bc) of the plan (n, q)."""
        if (n, q) not in self.cache:
            psi = numtheory.primitive_2n_root(n, q)
            lazy = self.lib.emu_is_lazy(n, q, psi)
            assert lazy in (0, 1), (n, q, lazy)
            self.cache[(n, q)] = (bool(lazy), self.lib.bc_enabled(n, q, psi) == 1)
        return self.cache[(n, q)]


def ntt_prime_above(limit, n):
    """smallest prime q > limit with q = 1 (mod 2n)"""
    q = limit // (2 * n) * (2 * n) + 1
    if q <= limit:
        q += 2 * n
    while not is_prime(q):
        q += 2 * n
    return q


def boundary(flag, n, k, walk):
    """(last prime with the flag, first without) among the NTT primes in (2^(k-1), 2^k) from the top; None if the largest prime
    below 2^k has not got it, or if every prime of k bits has."""
    top = ntt_prime_below(2 ** k, n)
    if top < 2 ** (k - 1) or not flag(n, top):
        return None
    if walk:
        q = top
        while True:
            nxt = ntt_prime_below(q, n)
            if nxt < 2 ** (k - 1):
                return None
            if not flag(n, nxt):
                return q, nxt
            q = nxt
    good, step = top, 2 * n
    while True:                                  # a prime without the flag: c doubles until one is found
        if good - step < 2 ** (k - 1):
            bad = ntt_prime_above(2 ** (k - 1), n)
            if flag(n, bad):
                return None
            break
        bad = ntt_prime_below(good - step, n)
        if bad < 2 ** (k - 1):
            return None
        if not flag(n, bad):
            break
        step *= 2
    while True:                                  # good has the flag, bad has not, bad < good
        mid = (good + bad) // 2
        q = ntt_prime_below(mid, n)
        if q <= bad:
            q = ntt_prime_above(mid - 1, n)
            if q >= good:
                return good, bad
        if flag(n, q):
            good = q
        else:
            bad = q


def flag_tables(flags, walk):
    """CG_PAIRS, CIN_PAIRS, MID_PAIRS and FLAG_ENTRIES.  A flag whose boundary is the lazy policy's at that word length has no pair
    of its own (cg_lazy everywhere; cg_sched and cin at k <= 55): the self-check asserts that it equals lazy there."""
    n = 4096
    tables = {"cg_lazy": [], "cg_sched": [], "cin": []}
    entries = {(n, Q60)}
    for k in K_BOUNDARY:
        lazy = boundary(flags.has("lazy"), n, k, walk)
        for name, found in tables.items():
            pair = boundary(flags.has(name), n, k, walk)
            if pair is None:                         # 32-bit lanes (or no lazy prime of k bits): the flag is never set
                assert lazy is None or not any(flags.has(name)(n, q) for q in lazy), (name, k)
            elif pair != lazy:
                found.append((n, name) + pair)
                entries.update((n, q) for q in pair)
        if k in K_FLAGS:
            entries.update((n, q) for q in lazy + boundary(flags.has("bc"), n, k, walk))
    assert not tables["cg_lazy"], tables["cg_lazy"]          # never tighter than lazy with 64-bit lanes
    mid = []
    for m in MID_N:
        for k in MID_K:
            pair = boundary(flags.has("lazy"), m, k, walk)
            mid.append((m, "lazy") + pair)
            entries.update((m, q) for q in pair)
    for name, rows in (("CG_PAIRS", tables["cg_sched"]), ("CIN_PAIRS", tables["cin"]), ("MID_PAIRS", mid)):
        print(f"{name} = [")
        for p in rows:
            print(f"    ({p[0]}, \"{p[1]}\", {p[2]}, {p[3]}),")
        print("]")
    print("# (n, q, " + ", ".join(FLAG_NAMES) + ")")
    print("FLAG_ENTRIES = [")
    for n_, q in sorted(entries):
        print(f"    ({n_}, {q}, " + ", ".join(str(f) for f in flags.mask(n_, q)) + "),")
    print("]")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[256, 4096, 8192])
    ap.add_argument("--walk", action="store_true", help="visit every NTT prime from 2^k downwards instead of bisecting")
    ap.add_argument("--tables", choices=("all", "policy", "flags"), default="all",
                    help="policy: PAIRS and ENTRIES; flags: CG_PAIRS, CIN_PAIRS, MID_PAIRS and FLAG_ENTRIES (n = 512 ... 4096, whatever --n says)")
    args = ap.parse_args()
    flags = Flags()
    if args.tables != "flags":
        policy_tables(flags, args)
    if args.tables != "policy":
        flag_tables(flags, args.walk)


def policy_tables(flags, args):
    pairs, entries = [], []

    def add(n, q):
        if (n, q) not in [(e[0], e[1]) for e in entries]:
            entries.append((n, q) + flags(n, q))

    for n in args.n:
        for k in K_BOUNDARY:
            found = boundary(lambda n_, q: flags(n_, q)[0], n, k, args.walk)
            if found is None:
                add(n, ntt_prime_below(2 ** k, n))               # e.g. the largest prime below 2^28: not lazy
                continue
            pairs.append((n, "lazy") + found)
            add(n, found[0]); add(n, found[1])
            bc = boundary(lambda n_, q: flags(n_, q)[1], n, k, args.walk)
            if bc is not None:
                pairs.append((n, "bc") + bc)
                add(n, bc[0]); add(n, bc[1])
        for k in K_WORD:
            for limit in (2 ** k, int(0.71 * 2 ** k)):
                add(n, ntt_prime_below(limit, n))
    for n, q in REFERENCE:
        if n in args.n:
            add(n, q)

    print("# (n, flag, last prime = 1 (mod 2n) with the flag walking down from 2^k, first without it)")
    print("PAIRS = [")
    for p in pairs:
        print(f"    ({p[0]}, \"{p[1]}\", {p[2]}, {p[3]}),")
    print("]")
    print("# (n, q, lazy, bc)")
    print("ENTRIES = [")
    for e in sorted(entries):
        print(f"    ({e[0]}, {e[1]}, {e[2]}, {e[3]}),")
    print("]")


if __name__ == "__main__":
    main()
