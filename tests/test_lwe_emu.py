"""CPU stepping of the three LWE kernels (tests/emu_lwe/emu_lwe.cpp: lwe_modswitch_kernel, lwe_sample_extract_kernel and
lwe_keyswitch_kernel stepped tile by tile with the kernels' own header, tiny_ntt_amd/csrc/lwe_core.h) against the statements in
Python integers of tests/lwe_cases.py, against identities that use none of the project's arithmetic (the phase of an extracted
ciphertext, a trivial key), with guard words around every output, and the sanitizer program, without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import lwe_cases as L
from lwe_cases import EVEN_COMPOSITE, KS_SHAPES, MODSWITCH_MODULI, Q23, Q60, Q62, WORD_SIZE

MODES = (False, True)                      # unsigned, balanced
KS_MODULI = (Q23, WORD_SIZE[0], WORD_SIZE[1], Q62)


@pytest.fixture(scope="module")
def emu():
    return L.emu_lwe()


# ---- modulus switch --------------------------------------------------------------------------------
@pytest.mark.parametrize("q", MODSWITCH_MODULI, ids=[f"q{q}" for q in MODSWITCH_MODULI])
def test_modswitch_is_the_rounding_in_python_integers(emu, q):
    """n = 256, dim in {1, 5, 16}, batch in {1, 7}; 0, q - 1, q, the all-ones word and both sides of rounding boundaries among the
    words; the largest prime below 2^62 and an even composite modulus among the moduli."""
    n = 256
    assert L.has_all_edges(L.modswitch_rows(q, n, 7, 5), q, n) and L.has_all_edges(L.modswitch_rows(q, n, 7, 16), q, n)
    for dim in (1, 5, 16):
        for batch in (1, 7):
            lwe = L.modswitch_rows(q, n, batch, dim)
            words = set(int(v) for v in lwe.reshape(-1))
            assert set(L.special_words(q)[:lwe.size]) <= words and (lwe.size < 30 or L.has_all_edges(lwe, q, n))
            got, intact = emu.modswitch(n, q, lwe)
            assert intact
            assert got.shape == (dim + 1, batch) and np.array_equal(got, L.modswitch(lwe, q, n)), (dim, batch)


@pytest.mark.parametrize("q", MODSWITCH_MODULI, ids=[f"q{q}" for q in MODSWITCH_MODULI])
def test_modswitch_edges_word_by_word(emu, q):
    """Every edge word in one launch whose tiles are ragged on both sides (70 rows of 67 words), at n = 256 and at n = 4, 8192."""
    for n in (4, 256, 8192):
        edges = L.edge_words(q, n)
        lwe = np.array(edges + [0] * (70 * 67 - len(edges)), dtype=np.uint64).reshape(70, 67)
        assert L.has_all_edges(lwe, q, n) and set(L.special_words(q)) <= set(edges)
        got, intact = emu.modswitch(n, q, lwe)
        assert intact and np.array_equal(got, L.modswitch(lwe, q, n)), n
        assert int(got.max()) < 2 * n
    top = np.array([[q - 1, q]], dtype=np.uint64)                  # q - 1 rounds to 2n, which is 0 mod 2n; q is 0
    got, _ = emu.modswitch(256, q, top)
    assert got.ravel().tolist() == [0, 0]


# ---- sample extraction -------------------------------------------------------------------------------
def schoolbook_coefficient(c1, s, q, index):
    """Coefficient `index` of c1 * s in Z_q[x] / (x^n + 1), Python integers."""
    n, acc = len(c1), 0
    for i in range(n):
        j = index - i
        acc += int(c1[i]) * int(s[j]) if j >= 0 else -int(c1[i]) * int(s[j + n])
    return acc % q


@pytest.mark.parametrize("q", [Q23, WORD_SIZE[1], Q62, EVEN_COMPOSITE])
@pytest.mark.parametrize("n", [4, 256])
def test_sample_extract_is_the_statement_and_its_phase_is_the_coefficient(emu, q, n):
    rng = np.random.default_rng(n + q % 1000)
    for batch in (1, 5):
        a = L.extract_rows(q, n, batch)
        s = rng.integers(0, q, n, dtype=np.uint64)
        for index in (0, 1, n // 2, n - 1):
            got, intact = emu.sample_extract(n, q, a, index)
            assert intact
            assert np.array_equal(got, L.sample_extract(a, q, index)), (batch, index)
            assert int(got.max()) < q
            for r in range(batch):                       # an identity of its own: the phase is that coefficient of c0 + c1 s
                phase = (int(got[r, n]) + sum(int(x) * int(y) for x, y in zip(got[r, :n], s))) % q
                c1 = [int(v) % q for v in a[r, 1]]
                assert phase == (int(a[r, 0, index]) % q + schoolbook_coefficient(c1, s, q, index)) % q, (batch, index, r)


def test_sample_extract_rows_of_a_tile_and_past_it(emu):
    """n = 256: four rows per tile; 4, 5 and 9 rows end on a tile, past one, past two."""
    q, n = Q60, 256
    for batch in (4, 5, 9):
        a = L.extract_rows(q, n, batch)
        got, intact = emu.sample_extract(n, q, a, 77)
        assert intact and np.array_equal(got, L.sample_extract(a, q, 77)), batch


# ---- key switch --------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", KS_MODULI, ids=[f"q{q}" for q in KS_MODULI])
@pytest.mark.parametrize("shape", KS_SHAPES, ids=[f"{a}x{b}" for a, b in KS_SHAPES])
def test_keyswitch_is_the_product_in_python_integers(emu, q, shape):
    """Batch 1, 7 and R + 1 (rows are independent: the smaller batches are the first rows of the largest), both digit modes, the
    gadget tests' (terms, w) pairs and w = 32 on a 64-bit plan."""
    n_in, n_out = shape
    for terms, w in L.ks_pairs(q):
        for balanced in MODES:
            lwe, ksk, want = L.ks_reference(q, n_in, n_out, terms, w, balanced, emu.R + 1)
            for batch in (1, 7, emu.R + 1):
                got, intact = emu.keyswitch(q, lwe[:batch], ksk, terms, w, balanced)
                assert intact
                assert np.array_equal(got, want[:batch]), (terms, w, balanced, batch)


@pytest.mark.parametrize("q", [WORD_SIZE[0], WORD_SIZE[1], Q62], ids=["32-bit-lanes", "q4294962689", "q62"])
def test_keyswitch_accumulator_worst_case(emu, q):
    """n_in = 4096, terms = 2, the largest w the modulus allows (30, 31, 32), every digit at its largest, every key word q - 1: a sum
    kept in too few bits fails here."""
    lwe, ksk, terms, w = L.worst_case(q)
    assert w == {WORD_SIZE[0]: 30, WORD_SIZE[1]: 31, Q62: 32}[q]
    for balanced in MODES:
        got, intact = emu.keyswitch(q, lwe, ksk, terms, w, balanced)
        assert intact and np.array_equal(got, L.keyswitch(lwe, ksk, q, terms, w, balanced)), balanced
    # a balanced low digit at its largest magnitude, -B/2, against key words 1: q - 1 is what the kernel multiplies it by
    x = (1 << (w - 1)) + (max((q >> w) - 2, 0) << w)
    assert x < q and L.signed_digits(x, q, terms, w, True)[0] == -(1 << (w - 1))
    lwe, ksk = np.full_like(lwe, x), np.ones_like(ksk)
    got, intact = emu.keyswitch(q, lwe, ksk, terms, w, True)
    assert intact and np.array_equal(got, L.keyswitch(lwe, ksk, q, terms, w, True))


@pytest.mark.parametrize("q,terms,w", [(Q23, 3, 8), (WORD_SIZE[0], 4, 8), (Q60, 4, 15), (Q62, 2, 31)])
def test_trivial_key_returns_the_input(emu, q, terms, w):
    """ksk[i][j][k] = B^j [k == i], unsigned digits that cover q: the output is the input mod q.  None of the project's arithmetic
    stands on the expected side."""
    n = 40
    rng = np.random.default_rng(q % 977)
    lwe = L.any_words(rng, q, (emu.R + 1, n + 1))
    lwe[0, :3] = (0, q, q - 1)
    got, intact = emu.keyswitch(q, lwe, L.trivial_key(q, n, terms, w), terms, w, False)
    assert intact and np.array_equal(got, lwe % np.uint64(q))


def test_sanitizer_program_runs_clean():
    """The stepping's cases (tests/emu_lwe/emu_lwe.cpp, behind EMU_SANITIZE_CASES) under AddressSanitizer + UBSan, once: the three
    steppings on exactly sized buffers at four moduli against 128-bit host arithmetic, and the argument lists on made-up addresses.
    A stand-alone program of its own (tests/emu_lwe/sanitize_lwe.cpp): nothing is loaded into Python."""
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu_lwe")
    b = subprocess.run(["make", "-j8", "-C", d, "sanitize"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout[-2000:]
    r = subprocess.run([os.path.join(d, "_build", "sanitize_lwe")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    counts = {name: int(v) for name, v in re.findall(r"^(\w+): (\d+) checks$", r.stdout, re.M)}
    assert counts == {"lwe": 376}, counts
    assert re.search(r"^sanitize_lwe: 376 checks, 0 failures$", r.stdout, re.M), r.stdout[-500:]
