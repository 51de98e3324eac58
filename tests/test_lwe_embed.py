"""CPU stepping of the LWE embedding (tests/emu_pack/emu_pack.cpp: lwe_embed_kernel's per-thread code, lwe_core.h's lwe_embed_words,
over a grid of three workgroups) against a numpy statement of the definition in include/tinyntt.h, as the inverse of the stepped
sample extraction (tests/emu_lwe), and the entry point's argument list (csrc/api_checks.h: check_lwe_embed), without a GPU."""
import numpy as np
import pytest

from lwe_cases import MODSWITCH_MODULI, Q23, Q60, any_words, emu_lwe, lane_bits, sample_extract
from test_pack_emu import EmuPack

OK, EINVAL = 0, 6
FN = "tn_lwe_embed_dev"


@pytest.fixture(scope="module")
def pack():
    return EmuPack()


def embed_np(lwe, q, index):
    """lwe (batch, n + 1) of any words -> (batch, 2, n): c1[k] = lwe[index - k] for k <= index, -lwe[n + index - k] above it;
    c0[index] = lwe[n], 0 elsewhere; all mod q."""
    lwe = np.asarray(lwe, dtype=np.uint64)
    batch, n = lwe.shape[0], lwe.shape[1] - 1
    out = np.zeros((batch, 2, n), dtype=np.uint64)
    for r in range(batch):
        x = [int(v) % q for v in lwe[r]]
        for k in range(n):
            out[r, 1, k] = x[index - k] if k <= index else (q - x[n + index - k]) % q
        out[r, 0, index] = x[n]
    return out


def lwe_rows(q, n, batch, seed=5):
    """Words of the lane of any value, with 0, q - 1, q and the all-ones word at the ends of a row and in the body."""
    rng = np.random.default_rng(seed + n)
    lwe = any_words(rng, q, (batch, n + 1))
    full = 2 ** lane_bits(q) - 1
    lwe[0, :4] = (0, q - 1, q, full)
    lwe[0, n] = q
    lwe[-1, n - 2:] = (q, 0, full)
    return lwe


def indices(n):
    return [0, 1, n // 2, n - 1]


@pytest.mark.parametrize("q", MODSWITCH_MODULI, ids=[f"q{q.bit_length()}_{q % 1000}" for q in MODSWITCH_MODULI])
@pytest.mark.parametrize("n", [4, 256, 1024])
def test_stepped_embedding_is_the_definition(pack, n, q):
    """Every kind of modulus the LWE calls take (both lane widths, word-size moduli, a general plan's), batch 5: more words than
    one pass of the three workgroups at n = 256 and above, fewer at n = 4."""
    lwe = lwe_rows(q, n, 5)
    for index in indices(n):
        assert np.array_equal(pack.embed(n, q, lwe, index), embed_np(lwe, q, index)), (n, q, index)


@pytest.mark.parametrize("q", [Q23, Q60], ids=["q23", "q60"])
@pytest.mark.parametrize("n", [256, 1024])
def test_extraction_of_the_embedding_is_the_input_mod_q(pack, n, q):
    """sample_extract(embed(x), i) == x mod q for i in {0, 1, n - 1}: against the stepped extraction and its numpy statement.  At
    another index the extraction is a rotation of x by a monomial, not x."""
    lwe = lwe_rows(q, n, 3)
    want = lwe % np.uint64(q)
    for index in (0, 1, n - 1):
        a = pack.embed(n, q, lwe, index)
        got, intact = emu_lwe().sample_extract(n, q, a, index)
        assert intact and np.array_equal(got, want), (n, q, index)
        assert np.array_equal(sample_extract(a, q, index), want), (n, q, index)
    assert not np.array_equal(sample_extract(pack.embed(n, q, lwe, 1), q, 0), want)


def test_embedding_of_an_extraction_keeps_the_second_component_and_one_body_word(pack):
    """embed(sample_extract(a, i), i) has a's second component mod q and a's first at coefficient i alone."""
    n, q = 256, Q23
    a = any_words(np.random.default_rng(9), q, (2, 2, n))
    for index in (0, 7, n - 1):
        back = pack.embed(n, q, sample_extract(a, q, index), index)
        assert np.array_equal(back[:, 1], a[:, 1] % np.uint64(q))
        assert np.array_equal(back[:, 0, index], a[:, 0, index] % np.uint64(q)) and np.count_nonzero(np.delete(back[:, 0], index, axis=1)) == 0


# ---- the argument list -------------------------------------------------------------------------
N, WORD, Q = 4, 4, 7681
ANY, NULL = (N, WORD, 0, 1, Q), (0, 0, 0, 0, 0)          # every plan: an omega-only general plan stands for all
L, A = 1 << 20, 1 << 30
LWE_BYTES, A_BYTES = (N + 1) * WORD, 2 * N * WORD
T_OVERLAP = FN + ": output must not alias or overlap the input"

TABLE = [
    ("ok", ANY, L, A, dict(batch=3, index=N - 1), OK, None, True),
    ("null-plan", NULL, L, A, dict(batch=3), EINVAL, FN + ": plan is NULL", False),
    ("index-n", ANY, L, A, dict(batch=3, index=N), EINVAL, FN + ": index must be below n", False),
    ("words-2^31", ANY, L, A, dict(batch=(2 ** 31) // (N + 1) + 1), EINVAL, FN + ": batch * (n + 1) too large for one call (max 2^31 - 1 words)", False),
    ("batch0-null", ANY, None, None, dict(batch=0), OK, None, False),
    ("null-lwe", ANY, None, A, dict(batch=3), EINVAL, FN + ": NULL buffer", False),
    ("null-a", ANY, L, None, dict(batch=3), EINVAL, FN + ": NULL buffer", False),
    ("a-is-lwe", ANY, L, L, dict(batch=3), EINVAL, T_OVERLAP, False),
    ("a-over-last-byte-of-lwe", ANY, L, L + 3 * LWE_BYTES - 1, dict(batch=3), EINVAL, T_OVERLAP, False),
    ("a-just-past-lwe", ANY, L, L + 3 * LWE_BYTES, dict(batch=3), OK, None, True),
    ("a-last-byte-is-first-of-lwe", ANY, L, L - 3 * A_BYTES + 1, dict(batch=3), EINVAL, T_OVERLAP, False),
    ("a-just-before-lwe", ANY, L, L - 3 * A_BYTES, dict(batch=3), OK, None, True),
    ("null-plan-index-n", NULL, L, A, dict(batch=3, index=N), EINVAL, FN + ": plan is NULL", False),
    ("index-n-batch-0", ANY, None, None, dict(batch=0, index=N), EINVAL, FN + ": index must be below n", False),
    ("index-n-null-a", ANY, L, None, dict(batch=3, index=N), EINVAL, FN + ": index must be below n", False),
]


@pytest.mark.parametrize("row", TABLE, ids=[r[0] for r in TABLE])
def test_argument_list(pack, row):
    _, view, lwe, a, kw, status, text, launches = row
    st, got, goes_on = pack.check_embed(view, lwe, a, **kw)
    assert (st, goes_on) == (status, launches), (st, got, goes_on)
    assert got == (text or ""), got
