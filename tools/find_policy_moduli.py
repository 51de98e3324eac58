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
tests/test_policy_moduli_emu.py::test_table_flags_and_boundary_pairs re-checks every literal in one prime step per pair."""
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


class Flags:
    def __init__(self):
        import ctypes
        self.lib = Emu().lib
        self.lib.bc_enabled.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]
        self.cache = {}

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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=int, nargs="+", default=[256, 4096, 8192])
    ap.add_argument("--walk", action="store_true", help="visit every NTT prime from 2^k downwards instead of bisecting")
    args = ap.parse_args()
    flags = Flags()
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
