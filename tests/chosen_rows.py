"""Operand rows with CHOSEN spectra and rows at the fold boundaries, shared by tests/test_emu.py (CPU stepping) and
tests/test_gpu_parity.py (the kernels).  Forward-transform outputs of random rows are uniformly random, so the pointwise
product and the base case never see spectra of 0, 1 or q - 1, and the load step never sees q, 2q, 2^k or the largest multiple
of q in the word.  Here the spectrum is picked first and the row is its inverse transform, computed with the oracle."""
import numpy as np

# every fused shape: (n, q); the reference plans' psi comes from conftest.PARAMS, the others' from numtheory
Q23, Q60 = 8380417, 1152921504606830593
SHAPES = [(256, Q23), (512, Q23), (1024, Q23), (2048, Q23), (4096, Q23), (512, Q60), (2048, Q60), (4096, Q60), (8192, Q60)]


def psi_of(n, q):
    from conftest import PARAMS
    from tiny_ntt_amd import numtheory
    for pn, pq, ppsi in PARAMS.values():
        if (pn, pq) == (n, q):
            return ppsi
    return numtheory.primitive_2n_root(n, q)


def spectra(n, q, rng):
    """Rows of spectrum entries from {0, 1, 2, (q-1)/2, (q+1)/2, q-2, q-1}: constant rows; equal and opposite (e, q - e) within the
    index pairs (2i, 2i+1) and (i, i + n/2) - one of the two is the pair of a last-stage butterfly whatever the output order, so the
    base case sees residues (e, 0) and (0, .); seeded random picks."""
    vals = np.array([0, 1, 2, (q - 1) // 2, (q + 1) // 2, q - 2, q - 1], dtype=np.uint64)
    rows = [np.full(n, v, dtype=np.uint64) for v in vals]
    for opposite in (False, True):
        e = vals[rng.integers(0, len(vals), n // 2)]
        f = (np.uint64(q) - e) % np.uint64(q) if opposite else e
        rows.append(np.stack([e, f], axis=1).reshape(n))           # pairs (2i, 2i+1)
        rows.append(np.concatenate([e, f]))                          # pairs (i, i + n/2)
    for _ in range(3):
        rows.append(vals[rng.integers(0, len(vals), n)])
    return np.stack(rows)


def rows_of_spectra(oracle, S, n, q, psi):
    """a with twist + cg_ntt(a) == S: the untwisted cg_intt of S (asserted by transforming back)."""
    omega = psi * psi % q
    psi_inv = pow(psi, q - 2, q)
    tw = np.array([pow(psi, i, q) for i in range(n)], dtype=object)
    utw = np.array([pow(psi_inv, i, q) for i in range(n)], dtype=object)
    out = np.empty_like(S)
    for r in range(S.shape[0]):
        a = oracle.cg_intt(S[r], omega, q).astype(object) * utw % q
        assert np.array_equal(oracle.cg_ntt((a * tw % q).astype(np.uint64), omega, q), S[r])
        out[r] = a.astype(np.uint64)
    return out


def boundary_values(q, word):
    k = q.bit_length()
    top = (word - 1) // q * q
    return [v for v in (q, q + 1, 2 * q - 1, 2 * q, 2 ** k - 1, 2 ** k, 2 ** k + 1, word // 2, top, top - 1, top + 1) if v < word]


class ChosenRows:
    """a, b: the operand rows (at most 64); nspec: rows [0, 2 nspec) are chosen-spectrum rows (the second half their unreduced
    twins a + j q, j the largest that fits the lane word) with spectra Sa, Sb; the rest are boundary rows."""

    def __init__(self, oracle, n, q, psi, seed=2024):
        rng = np.random.default_rng(seed)
        word = 2 ** 32 if q < 2 ** 31 else 2 ** 64
        S = spectra(n, q, rng)
        m = S.shape[0]
        self.Sa, self.Sb = S, S[(3 * np.arange(m) + 1) % m]
        a, b = rows_of_spectra(oracle, self.Sa, n, q, psi), rows_of_spectra(oracle, self.Sb, n, q, psi)
        lift = lambda x: (x.astype(object) + (word - 1 - x.astype(object)) // q * q).astype(np.uint64)
        bv = boundary_values(q, word)
        B = np.stack([np.full(n, v, dtype=np.uint64) for v in bv])
        R = rng.integers(0, q, B.shape, dtype=np.uint64)
        self.nspec = m
        self.a = np.concatenate([a, lift(a), B, B])
        self.b = np.concatenate([b, lift(b), R, B])
        assert self.a.shape[0] <= 64 and self.a.astype(object).max() < word and (lift(a) % np.uint64(q) == a).all()
        self.ref = oracle.poly_mult(self.a, self.b, q, psi)
        omega = psi * psi % q
        self.fwd = np.stack([oracle.cg_ntt(r, omega, q) for r in self.a])      # cg_ntt / cg_intt of the same rows
        self.inv = np.stack([oracle.cg_intt(r, omega, q) for r in self.a])
        # the spectra were chosen: the product's spectrum is their entrywise product, whatever the oracle's product says
        Sc = (self.Sa.astype(object) * self.Sb.astype(object) % q).astype(np.uint64)
        assert np.array_equal(rows_of_spectra(oracle, Sc, n, q, psi), self.ref[:m]) and np.array_equal(self.ref[m:2 * m], self.ref[:m])


_CACHE = {}


def chosen_rows(oracle, n, q):
    """Computed once per shape and shared; callers must not modify the arrays."""
    if (n, q) not in _CACHE:
        c = _CACHE[(n, q)] = ChosenRows(oracle, n, q, psi_of(n, q))
        for arr in (c.a, c.b, c.ref, c.fwd, c.inv, c.Sa, c.Sb):
            arr.setflags(write=False)
    return _CACHE[(n, q)]
