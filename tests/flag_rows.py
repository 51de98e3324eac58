"""Operand rows and their oracle results for the moduli of policy_moduli.FLAG_ENTRIES, shared by tests/test_policy_flags_emu.py
(CPU stepping) and tests/test_gpu_policy_flags.py (the kernels).  Per modulus: the rows of test_prepared_emu.operand_rows (unreduced
random words, all q - 1, x^(n-1) * x), then (chosen=True) the rows of tests/chosen_rows.py (chosen spectra, their unreduced twins,
fold-boundary rows), and four more inputs for the inverse transforms only: a row of full-width random words, of q, of 2q - 1 and of
2^k.  Every expected value comes from the oracle on the rows REDUCED mod q (any word is taken mod q): the product, cg_ntt, cg_ntt of
the twisted row, cg_intt, and the cyclic product composed as forward transforms, entrywise product in Python integers, inverse."""
import numpy as np

from chosen_rows import chosen_rows, psi_of
from test_prepared_emu import operand_rows

PLAIN = 5                  # rows [0, PLAIN) are operand_rows; row 3 is all q - 1


class FlagRows:
    def __init__(self, oracle, n, q, chosen):
        psi = psi_of(n, q)
        omega = psi * psi % q
        Q = np.uint64(q)
        word = 2 ** 32 if q < 2 ** 31 else 2 ** 64
        a, b = operand_rows(n, q, n + q % 1000)
        if chosen:
            cr = chosen_rows(oracle, n, q)
            a, b = np.concatenate([a, cr.a]), np.concatenate([b, cr.b])
        self.n, self.q, self.psi, self.a, self.b = n, q, psi, a, b
        ra, rb = a % Q, b % Q
        self.ra, self.rb = ra, rb
        self.prod = oracle.poly_mult(ra, rb, q, psi)
        self.fwd = np.stack([oracle.cg_ntt(r, omega, q) for r in ra])
        fwd_b = np.stack([oracle.cg_ntt(r, omega, q) for r in rb])
        twist = np.array([pow(psi, i, q) for i in range(n)], dtype=object)
        self.tfwd = np.stack([oracle.cg_ntt((r.astype(object) * twist % q).astype(np.uint64), omega, q) for r in ra])
        spec = (self.fwd.astype(object) * fwd_b.astype(object) % q).astype(np.uint64)
        self.cyc = np.stack([oracle.cg_intt(r, omega, q) for r in spec])
        rng = np.random.default_rng(q % 1000 + 1)
        extra = np.stack([rng.integers(0, word - 1, n, dtype=np.uint64, endpoint=True)] +
                         [np.full(n, v, dtype=np.uint64) for v in (q, 2 * q - 1, 2 ** q.bit_length())])
        assert 2 ** q.bit_length() < word and int(extra[0].max()) >= 2 * q
        self.x = np.concatenate([a, extra])                         # inputs of the inverse transforms
        self.inv = np.stack([oracle.cg_intt(r, omega, q) for r in self.x % Q])
        assert self.prod[4, 0] == q - 1 and not self.prod[4, 1:].any()      # x^(n-1) * x = -1
        if chosen:            # the oracle takes unreduced rows mod q too: chosen_rows.py's results are those of the reduced rows
            assert np.array_equal(self.prod[PLAIN:], cr.ref) and np.array_equal(self.fwd[PLAIN:], cr.fwd)
            assert np.array_equal(self.inv[PLAIN:PLAIN + cr.a.shape[0]], cr.inv)
            assert np.array_equal(self.tfwd[PLAIN:PLAIN + cr.nspec], cr.Sa)
        for arr in (self.a, self.b, self.ra, self.rb, self.prod, self.fwd, self.tfwd, self.cyc, self.x, self.inv):
            arr.setflags(write=False)


_CACHE = {}


def flag_rows(oracle, n, q, chosen=True):
    """Computed once per modulus and shared; callers must not modify the arrays."""
    if (n, q, chosen) not in _CACHE:
        _CACHE[(n, q, chosen)] = FlagRows(oracle, n, q, chosen)
    return _CACHE[(n, q, chosen)]
