"""The matrix-core key switch on the CPU: the limb rule in Python integers, the stepped key preparation
(tests/emu_lwe_mfma/emu_lwe_mfma.cpp steps lwe_ksk_prepare_kernel from tiny_ntt_amd/csrc/lwe_mfma_core.h) read back through the
layout rule, the stepped key switch against tests/lwe_cases.py's statement at every edge of the tile code, the fold of the 32-bit
sums past 2^31, the host loop of the matrix step against the product written out, the bank rule of the digit image's reads, and
the stepping's cases as a stand-alone program under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import lwe_cases as L
import lwe_mfma_cases as M
from conftest import ROOT, _make
from test_lds_banks import conflict_degree


@pytest.fixture(scope="module")
def emu():
    return M.emu_lwe_mfma()


def test_geometry_is_the_shared_one(emu):
    assert (emu.ROWS, emu.COLS, emu.K_STEP, emu.CHUNK, emu.COL_TILE) == (M.ROWS, M.COLS, M.K_STEP, M.CHUNK, M.COL_TILE)
    assert emu.FLUSH_PRODUCTS == 2 ** 16 and emu.FLUSH_PRODUCTS * 2 ** 14 <= 2 ** 31 - 1 < 2 * emu.FLUSH_PRODUCTS * 2 ** 14
    assert emu.FLUSH_PRODUCTS % emu.CHUNK == 0 and emu.CHUNK % emu.K_STEP == 0


def limb_words(q):
    rng = np.random.default_rng(q % 1000)
    full = 2 ** L.lane_bits(q) - 1
    return [0, 1, q // 2, q // 2 + 1, q - 1, q, min(q + 1, full), full] + [int(v) for v in L.any_words(rng, q, 40)]


@pytest.mark.parametrize("q", M.MODULI, ids=[f"q{q}" for q in M.MODULI])
def test_limb_rule_in_python_integers(emu, q):
    """Every limb in [-128, 128), sum s_l 256^l the centred residue, L(q) minimal and the header's; the words 0, 1, floor(q / 2),
    floor(q / 2) + 1, q - 1 and any words from q on."""
    count = M.limb_count(q)
    assert count == emu.limbs(q)
    for x in limb_words(q):
        s = M.limbs_of(x, q, count)
        c = M.centred(x, q)
        assert all(-128 <= v < 128 for v in s) and sum(v * 256 ** l for l, v in enumerate(s)) == c and -q < 2 * c <= q, x
        assert (c - int(x)) % q == 0
    S = (256 ** (count - 1) - 1) // 255                       # one limb fewer misses the largest centred residue
    assert q // 2 > 127 * S
    assert {L.Q23: 3, L.Q60: 8}.get(q, count) == count
    if q == L.Q23:
        assert 127 * (2 ** 24 - 1) // 255 == 8355711 < q - 1  # the canonical residue would not fit 3 limbs: the centring is needed


@pytest.mark.parametrize("q", M.MODULI, ids=[f"q{q}" for q in M.MODULI])
def test_prepared_key_holds_the_limbs_and_zero_padding(emu, q):
    count = M.limb_count(q)
    for n_in, terms, n_out in ((1, 1, 1), (13, 5, 16), (3, 43, 64)):
        rng = np.random.default_rng(n_in)
        ksk = L.any_words(rng, q, (n_in, terms, n_out + 1))
        flat = ksk.reshape(-1)
        edge = limb_words(q)[:min(8, flat.size)]
        flat[:len(edge)] = edge
        kprep, intact = emu.prepare(q, ksk)
        assert intact and kprep.size == M.prepared_bytes(q, n_in, n_out, terms) == emu.bytes(q, n_in, n_out, terms)
        got = M.read_prepared(kprep, q, n_in, n_out, terms)
        want = np.zeros(got.shape, dtype=np.int8)
        k2 = ksk.reshape(n_in * terms, n_out + 1)
        for k in range(n_in * terms):
            for c in range(n_out + 1):
                want[k, c] = M.limbs_of(k2[k, c], q, count)
        assert np.array_equal(got, want)                       # the padding rows and columns of `want` are zero
        assert kprep[M.key_offset(n_in * terms - 1, n_out, count - 1, n_in, terms, count)].view(np.int8) == want[n_in * terms - 1, n_out, count - 1]


def check_case(emu, q, case):
    batch, n_in, n_out, terms, w, balanced = case
    lwe, ksk, want = L.ks_reference(q, n_in, n_out, terms, w, balanced, batch)
    got, intact = emu.keyswitch(q, lwe, ksk, terms, w, balanced)
    assert intact, case
    assert np.array_equal(got, want), case


@pytest.mark.parametrize("q", M.MODULI, ids=[f"q{q}" for q in M.MODULI])
def test_stepped_keyswitch_equals_the_statement(emu, q):
    """Both digit modes; every edge of the tile code at q = 8380417 (3 limbs, 32-bit lanes) and 2^60 - 2^14 + 1 (8 limbs), the
    byte-wide pairs and one case per dimension at the others."""
    cases = M.edge_cases(q, full=q in (L.Q23, L.Q60))
    assert {c[5] for c in cases} == {False, True}
    for case in cases:
        check_case(emu, q, case)


def test_stepped_keyswitch_equals_the_plain_stepping(emu):
    """... and the stepping of lwe_keyswitch_kernel, word for word (the contract of the C ABI)."""
    plain = L.emu_lwe()
    for q in (L.Q23, L.Q60):
        for case in M.edge_cases(q, full=False):
            batch, n_in, n_out, terms, w, balanced = case
            lwe, ksk, _ = L.ks_reference(q, n_in, n_out, terms, w, balanced, batch)
            assert np.array_equal(emu.keyswitch(q, lwe, ksk, terms, w, balanced)[0], plain.keyswitch(q, lwe, ksk, terms, w, balanced)[0]), case


def test_fold_keeps_sums_past_2_31_exact(emu):
    """131,136 products of 2^14 in every low-limb sum: a kernel that never folds, or folds too late, fails here and nowhere else."""
    lwe, ksk, want = M.flush_case(16)
    got, intact = emu.keyswitch(M.FLUSH_Q, lwe, ksk, M.FLUSH_TERMS, M.FLUSH_W, True, kprep=M.stepped_flush_key())
    assert intact and np.array_equal(got, want)
    one = L.keyswitch(lwe[:1, :], ksk[:, :, 14:], M.FLUSH_Q, M.FLUSH_TERMS, M.FLUSH_W, True)      # the closed form against the statement
    assert np.array_equal(one, want[:1, 14:])


def test_host_loop_of_the_matrix_step(emu):
    """The header's host loop against the map restated in Python: one-hot A against one-hot B, random asymmetric bytes with -128
    and 127 among them, from a non-zero accumulator."""
    rng = np.random.default_rng(5)
    for row, k, col in ((0, 0, 0), (3, 37, 9), (15, 63, 15), (12, 16, 1)):
        a = np.zeros((64, 16), dtype=np.int8); b = np.zeros((64, 16), dtype=np.int8)
        a[row + 16 * (k // 16), k % 16] = -128
        b[col + 16 * (k // 16), k % 16] = 127
        c = rng.integers(-1000, 1000, size=(64, 4), dtype=np.int32)
        want = c.copy()
        want[col + 16 * (row // 4), row % 4] += -128 * 127
        got = emu.step(a, b, c)
        assert np.array_equal(got, want) and np.array_equal(got, M.matrix_step(a, b, c))
    a = rng.integers(-128, 128, size=(64, 16), dtype=np.int8); b = rng.integers(-128, 128, size=(64, 16), dtype=np.int8)
    a[0, 0], a[1, 1], b[0, 0], b[2, 3] = -128, 127, -128, 127
    c = rng.integers(-2 ** 20, 2 ** 20, size=(64, 4), dtype=np.int32)
    assert np.array_equal(emu.step(a, b, c), M.matrix_step(a, b, c))


def test_digit_image_reads_have_no_bank_conflict(emu):
    """A wave's read of an A fragment is one 16-byte word per lane (ds_read_b128) at consecutive addresses: by the bank model of
    tests/test_lds_banks.py no two lanes of a lane group meet in a bank, for every step of the image and every row tile."""
    for step in range(emu.CHUNK // emu.K_STEP):
        for rt in range(emu.ROWS // 16):
            addrs = [emu.lib.emu_lwe_mfma_a_frag_offset(step, rt, lane) for lane in range(64)]
            assert all(a % 16 == 0 and a + 16 <= emu.IMAGE for a in addrs) and len(set(addrs)) == 64
            assert conflict_degree(addrs, "read", 16) == 1, (step, rt)


def test_sanitizer_program_runs_clean():
    """make -C tests/emu_lwe_mfma sanitize, then the program: the stepping's cases under AddressSanitizer + UBSan on exactly sized
    buffers (a stand-alone program; nothing is loaded into Python under a sanitizer)."""
    _make("tests/emu_lwe_mfma", "sanitize")
    r = subprocess.run([os.path.join(ROOT, "tests", "emu_lwe_mfma", "_build", "sanitize_lwe_mfma")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and " 0 failures" in r.stdout, r.stdout[-2000:]
