"""The LWE calls (tn_lwe_modswitch_dev, tn_sample_extract_dev, tn_lwe_keyswitch_dev) stated in Python integers, independent of
tiny_ntt_amd/csrc/lwe_core.h, with the inputs, shapes and moduli that tests/test_lwe_emu.py (CPU stepping) and tests/test_gpu_lwe.py
(the kernels) share, and the handle of the stepping's library (tests/emu_lwe/_build/libemu_lwe.so).

Conventions (include/tinyntt.h): an LWE row is a_0 .. a_{d-1}, b with phase b + sum a_i s_i; an RLWE ciphertext is [2][n] with
phase c0 + c1 s; every input word is taken mod q; outputs are canonical residues."""
import ctypes
import functools
import os

import numpy as np

import emu_library
from conftest import P64, ROOT, _make, p64

P32 = ctypes.POINTER(ctypes.c_uint32)
GUARD = 0xA5A5A5A5A5A5A5A5                       # guard words in front of and behind every output
GUARD_WORDS = 64

Q23, Q60, Q62 = 8380417, (1 << 60) - (1 << 14) + 1, 4611686018427379201      # Q62: the largest prime below 2^62 of tests/policy_moduli.py
WORD_SIZE = (2147483137, 4294962689, 8589921281)                               # below 2^31 (32-bit lanes), 2^32 and 2^33 (64-bit lanes)
EVEN_COMPOSITE = (1 << 40) + 2 * 3 * 5 * 7                                     # a general plan's modulus
MODSWITCH_MODULI = (Q23, Q60) + WORD_SIZE + (Q62, EVEN_COMPOSITE)
KS_SHAPES = ((1, 1), (8, 5), (33, 256), (256, 16), (256, 300))                 # (n_in, n_out): 257 and 301 columns cross a slab of 256


def lane_bits(q):
    return 32 if q < 2 ** 31 else 64


# ---- the statements ---------------------------------------------------------------------------------
def modswitch(lwe, q, n):
    """lwe (batch, dim + 1) of any words -> exps (dim + 1, batch): floor((2n x + floor(q / 2)) / q) mod 2n, x the word mod q."""
    lwe = np.asarray(lwe, dtype=np.uint64)
    out = np.empty(lwe.shape[::-1], dtype=np.uint32)
    for r in range(lwe.shape[0]):
        for i in range(lwe.shape[1]):
            out[i, r] = ((2 * n * (int(lwe[r, i]) % q) + q // 2) // q) % (2 * n)
    return out


def sample_extract(a, q, index):
    """a (batch, 2, n) of any words -> (batch, n + 1)."""
    a = np.asarray(a, dtype=np.uint64)
    batch, _, n = a.shape
    out = np.empty((batch, n + 1), dtype=np.uint64)
    for r in range(batch):
        c0, c1 = [int(v) % q for v in a[r, 0]], [int(v) % q for v in a[r, 1]]
        for i in range(n):
            out[r, i] = c1[index - i] if i <= index else (q - c1[n + index - i]) % q
        out[r, n] = c0[index]
    return out


def signed_digits(x, q, terms, w, balanced):
    """The library's digits of the word x as signed integers: base 2^w, unsigned, or balanced in [-B/2, B/2) with the carry
    running up the digits and the last carry dropped."""
    xh, B, carry, out = int(x) % q, 1 << w, 0, []
    for j in range(terms):
        t = ((xh >> (j * w)) & (B - 1)) + carry
        carry = 1 if balanced and t >= B // 2 else 0
        out.append(t - B if carry else t)
    return out


def keyswitch(lwe, ksk, q, terms, w, balanced):
    """lwe (batch, n_in + 1), ksk (n_in, terms, n_out + 1), any words -> (batch, n_out + 1):
    out[r][k] = [k == n_out] b_r + sum_i sum_j d_j(a_r[i]) ksk[i][j][k] mod q, as one product of matrices of Python integers."""
    lwe, ksk = np.asarray(lwe, dtype=np.uint64), np.asarray(ksk, dtype=np.uint64)
    batch, n_in = lwe.shape[0], lwe.shape[1] - 1
    K = (ksk.reshape(n_in * terms, -1).astype(object)) % q
    D = np.array([[d for x in row[:n_in] for d in signed_digits(x, q, terms, w, balanced)] for row in lwe], dtype=object).reshape(batch, n_in * terms)
    out = D.dot(K)
    out[:, -1] += lwe[:, n_in].astype(object) % q
    return (out % q).astype(np.uint64)


# ---- inputs -------------------------------------------------------------------------------------------
def any_words(rng, q, shape):
    """Words of the plan's lane, of any value."""
    return rng.integers(0, 2 ** lane_bits(q) - 1, size=shape, dtype=np.uint64, endpoint=True)


def edge_words(q, n):
    """0, q - 1, q, the all-ones word and the words on either side of a few rounding boundaries (2t + 1) q / 4n of the modulus
    switch (the first word that rounds up to t + 1 and the one before it)."""
    full = 2 ** lane_bits(q) - 1
    words = [0, 1, q - 1, q, min(q + 1, full), full]
    for t in (0, 1, n - 1, n, 2 * n - 2, 2 * n - 1):
        first = -(-((t + 1) * q - q // 2) // (2 * n))      # the first x with 2n x + floor(q / 2) >= (t + 1) q: just above (2t + 1) q / 4n
        for x in (first - 2, first - 1, first, first + 1):
            if 0 <= x <= full:
                words.append(x)
    return words


def special_words(q):
    """0, q - 1, q and the all-ones word of the lane: the first words of edge_words."""
    return [0, q - 1, q, 2 ** lane_bits(q) - 1]


def modswitch_rows(q, n, batch, dim, seed=1):
    """Random words of the lane with the edge words among them: all of them, each at a slot of its own, where the shape has
    room (has_all_edges); else as many as fit, the special words first."""
    rng = np.random.default_rng(seed + dim * 131 + batch)
    lwe = any_words(rng, q, (batch, dim + 1))
    flat = lwe.reshape(-1)
    edges = special_words(q) + [x for x in edge_words(q, n) if x not in special_words(q)]
    if len(edges) <= flat.size:
        slots = rng.permutation(flat.size)[:len(edges)]             # distinct slots, spread over rows and columns
    else:
        slots = np.arange(flat.size)
    for pos, x in zip(slots, edges):
        flat[pos] = x
    return lwe


def has_all_edges(lwe, q, n):
    return set(edge_words(q, n)) <= set(int(v) for v in lwe.reshape(-1))


def extract_rows(q, n, batch, seed=2):
    rng = np.random.default_rng(seed + n)
    a = any_words(rng, q, (batch, 2, n))
    full = 2 ** lane_bits(q) - 1
    a[0, 1, :3] = (0, q, full)
    a[0, 0, :3] = (full, 0, q)
    a[-1, 1, -2:] = (0, q)
    return a


def ks_pairs(q):
    """The (terms, w) pairs of the key-switch tests: test_gadget_emu.gadget_pairs, and w = 32 where the modulus is above 2^32."""
    k = q.bit_length()
    pairs = [(2, -(-k // 2)), (3, -(-k // 3)), (5, 1), (2, min(k - 1, 32))]
    if q > 2 ** 33:
        pairs.append((2, 32))
    return [p for i, p in enumerate(pairs) if p[1] <= 32 and p not in pairs[:i]]


def ks_inputs(q, n_in, n_out, terms, batch, seed=3):
    rng = np.random.default_rng(seed + n_in * 1000 + n_out + terms)
    lwe = any_words(rng, q, (batch, n_in + 1))
    ksk = any_words(rng, q, (n_in, terms, n_out + 1))
    lwe.reshape(-1)[:3] = (q - 1, q, 0)[:min(3, lwe.size)]
    ksk.reshape(-1)[:2] = (q, q - 1)[:min(2, ksk.size)]
    return lwe, ksk


def worst_case(q):
    """One accumulator worst case of the element width: n_in = 4096, terms = 2, the largest w the modulus allows (at most 32),
    every digit at its largest magnitude, every key word q - 1, batch 1, n_out = 3 -> (lwe, ksk, terms, w, balanced)."""
    n_in, terms, n_out = 4096, 2, 3
    w = min(q.bit_length() - 1, 32)
    x = (1 << (2 * w)) - 1                                  # both unsigned digits B - 1
    if x >= q:
        x = ((q >> w) << w) - 1                             # the low digit B - 1 under the largest high digit below q
    assert 0 <= x < q and signed_digits(x, q, terms, w, False)[0] == (1 << w) - 1
    lwe = np.full((1, n_in + 1), x, dtype=np.uint64)
    lwe[0, n_in] = q - 1
    ksk = np.full((n_in, terms, n_out + 1), q - 1, dtype=np.uint64)
    return lwe, ksk, terms, w


def trivial_key(q, n, terms, w):
    """ksk[i][j][k] = B^j [k == i], n_out = n_in = n: unsigned digits that cover q recompose the input."""
    assert terms * w >= q.bit_length() and (1 << w) < q
    ksk = np.zeros((n, terms, n + 1), dtype=np.uint64)
    for j in range(terms):
        ksk[np.arange(n), j, np.arange(n)] = (1 << (j * w)) % q
    return ksk


def guarded(shape, dtype):
    """-> (the whole buffer, the view of `shape` between GUARD_WORDS guard words on either side)."""
    count = int(np.prod(shape))
    buf = np.full(count + 2 * GUARD_WORDS, GUARD & (2 ** (8 * np.dtype(dtype).itemsize) - 1), dtype=dtype)
    return buf, buf[GUARD_WORDS:GUARD_WORDS + count].reshape(shape)


def guards_intact(buf):
    g = buf.dtype.type(GUARD & (2 ** (8 * buf.dtype.itemsize) - 1))
    return bool((buf[:GUARD_WORDS] == g).all() and (buf[-GUARD_WORDS:] == g).all())


# ---- the stepping's library ---------------------------------------------------------------------------
class EmuLwe:
    """The entry points of tests/emu_lwe/emu_lwe.cpp in tests/emu_lwe/_build/libemu_lwe.so (brought up to date first)."""

    def __init__(self):
        _make("tests/emu_lwe")
        L = self.lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_lwe", "_build", "libemu_lwe.so"))
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        tail = [ctypes.POINTER(ci), ctypes.c_char_p, sz]
        L.emu_lwe_modswitch.argtypes = [u32, u64, P64, P32, sz, sz]
        L.emu_sample_extract.argtypes = [u32, u64, P64, P64, sz, u32]
        L.emu_lwe_keyswitch.argtypes = [u64, P64, P64, P64, sz, sz, sz, sz, u32, u32]
        L.emu_lwe_modswitch_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, sz, sz] + tail
        L.emu_sample_extract_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, sz, u32] + tail
        L.emu_lwe_keyswitch_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, vp, sz, sz, sz, sz, u32, u32] + tail
        L.emu_lwe_ks_rows.restype = u32
        L.emu_lwe_ks_cols.restype = u32
        self.R, self.COLS = int(L.emu_lwe_ks_rows()), int(L.emu_lwe_ks_cols())

    def modswitch(self, n, q, lwe):
        """-> (exps (dim + 1, batch), the guards around it are intact)."""
        lwe = np.ascontiguousarray(lwe, dtype=np.uint64)
        batch, dim = lwe.shape[0], lwe.shape[1] - 1
        buf, out = guarded((dim + 1, batch), np.uint32)
        rc = self.lib.emu_lwe_modswitch(n, q, p64(lwe), out.ctypes.data_as(P32), batch, dim)
        assert rc == 0, rc
        return out.copy(), guards_intact(buf)

    def sample_extract(self, n, q, a, index):
        a = np.ascontiguousarray(a, dtype=np.uint64)
        buf, out = guarded((a.shape[0], n + 1), np.uint64)
        rc = self.lib.emu_sample_extract(n, q, p64(a), out.ctypes.data_as(P64), a.shape[0], index)
        assert rc == 0, rc
        return out.copy(), guards_intact(buf)

    def keyswitch(self, q, lwe, ksk, terms, w, balanced):
        lwe, ksk = np.ascontiguousarray(lwe, dtype=np.uint64), np.ascontiguousarray(ksk, dtype=np.uint64)
        batch, n_in, n_out = lwe.shape[0], lwe.shape[1] - 1, ksk.shape[2] - 1
        assert ksk.shape == (n_in, terms, n_out + 1)
        buf, out = guarded((batch, n_out + 1), np.uint64)
        rc = self.lib.emu_lwe_keyswitch(q, p64(lwe), p64(ksk), out.ctypes.data_as(P64), batch, n_in, n_out, terms, w, int(balanced))
        assert rc == 0, rc
        return out.copy(), guards_intact(buf)

    def check(self, which, view, *args):
        """The argument list of entry point `which` ("modswitch", "extract", "keyswitch") on the plan view (n, elem_bytes, has_fused,
        omega_only, q) -> (status, text, goes on to a launch)."""
        entry = {"modswitch": self.lib.emu_lwe_modswitch_api_check, "extract": self.lib.emu_sample_extract_api_check,
                 "keyswitch": self.lib.emu_lwe_keyswitch_api_check}[which]
        return emu_library.api_check(entry, *view, *args)


@functools.lru_cache(maxsize=None)
def emu_lwe():
    return EmuLwe()


@functools.lru_cache(maxsize=None)
def ks_reference(q, n_in, n_out, terms, w, balanced, batch):
    """(lwe, ksk, the statement's output) of a key-switch case, computed once per process and shared (read only)."""
    lwe, ksk = ks_inputs(q, n_in, n_out, terms, batch)
    want = keyswitch(lwe, ksk, q, terms, w, balanced)
    for arr in (lwe, ksk, want):
        arr.setflags(write=False)
    return lwe, ksk, want
