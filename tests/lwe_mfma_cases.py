"""The matrix-core key switch (tn_lwe_ksk_prepared_bytes, tn_lwe_ksk_prepare_dev, tn_lwe_keyswitch_prepared_dev) stated in Python
integers, independent of tiny_ntt_amd/csrc/lwe_mfma_core.h: the limb rule, the layout rule of the prepared key and the lane ->
element map of one matrix step; the shapes and inputs that tests/test_lwe_mfma_emu.py (CPU stepping) and
tests/test_gpu_lwe_mfma.py (the kernels) share; and the handle of the stepping's library
(tests/emu_lwe_mfma/_build/libemu_lwe_mfma.so).  The key switch's own statement is tests/lwe_cases.py's keyswitch."""
import ctypes
import functools
import os

import numpy as np

import emu_library
import lwe_cases as L
from conftest import P64, ROOT, _make, p64

K_STEP, COL_TILE, LANES = 64, 16, 64                 # include/tinyntt.h: [column tile of 16][K step of 64][limb][64 lanes][16 bytes]
MODULI = (L.Q23, L.Q60, L.Q62) + L.WORD_SIZE + (L.EVEN_COMPOSITE,)


# ---- the statements -----------------------------------------------------------------------------------
def centred(x, q):
    """The residue of the word x in (-q/2, q/2]."""
    c = int(x) % q
    return c - q if c > q // 2 else c


def limb_count(q):
    """The smallest L whose balanced limbs hold every centred residue: L limbs in [-128, 128) reach -128 S .. 127 S, S = (256^L - 1) / 255."""
    count = 1
    while True:
        S = (256 ** count - 1) // 255
        if -128 * S <= centred(q // 2 + 1, q) and q // 2 <= 127 * S:
            return count
        count += 1


def limbs_of(x, q, count):
    """The balanced base-256 limbs of the centred residue of x, from the low end, each in [-128, 128)."""
    c, out = centred(x, q), []
    for _ in range(count):
        s = (c + 128) % 256 - 128
        out.append(s)
        c = (c - s) // 256
    assert c == 0, (x, q, count)
    return out


def prepared_bytes(q, n_in, n_out, terms):
    return -(-(n_out + 1) // COL_TILE) * -(-(n_in * terms) // K_STEP) * limb_count(q) * LANES * 16


def key_offset(k, col, limb, n_in, terms, count):
    """Byte offset of limb `limb` of key row k = i * terms + j, column col, in the prepared key."""
    steps = -(-(n_in * terms) // K_STEP)
    frag = ((col // COL_TILE) * steps + k // K_STEP) * count + limb
    lane = col % 16 + 16 * ((k % 64) // 16)
    return (frag * LANES + lane) * 16 + k % 16


def read_prepared(kprep, q, n_in, n_out, terms):
    """The prepared key as an array (padded key rows, padded columns, L) of limbs, gathered through key_offset."""
    count = limb_count(q)
    rows, cols = -(-(n_in * terms) // K_STEP) * K_STEP, -(-(n_out + 1) // COL_TILE) * COL_TILE
    k, c, l = np.meshgrid(np.arange(rows), np.arange(cols), np.arange(count), indexing="ij")
    steps = rows // K_STEP
    off = ((((c // COL_TILE) * steps + k // K_STEP) * count + l) * LANES + c % 16 + 16 * ((k % 64) // 16)) * 16 + k % 16
    return np.asarray(kprep).view(np.int8)[off]


def matrix_step(a, b, c):
    """One matrix step D = A B + C on (64, 16) int8 fragments a, b and (64, 4) int32 c, by the lane -> element map of
    lwe_mfma_core.h restated: A[row l & 15][k = 16 (l >> 4) + j], B[k = 16 (l >> 4) + j][col l & 15], D[row 4 (l >> 4) + e][col l & 15]."""
    A = np.zeros((16, 64), dtype=np.int64); B = np.zeros((64, 16), dtype=np.int64); C = np.zeros((16, 16), dtype=np.int64)
    for l in range(64):
        A[l & 15, 16 * (l >> 4):16 * (l >> 4) + 16] = a[l]
        B[16 * (l >> 4):16 * (l >> 4) + 16, l & 15] = b[l]
        C[4 * (l >> 4):4 * (l >> 4) + 4, l & 15] = c[l]
    D = A @ B + C
    return np.array([[D[4 * (l >> 4) + e, l & 15] for e in range(4)] for l in range(64)], dtype=np.int32)


# ---- shapes and inputs --------------------------------------------------------------------------------
def byte_pairs(q):
    """(terms, w, balanced) of lwe_cases.ks_pairs(q) whose digits fit a signed byte (w <= 7, or <= 8 balanced); one pair per
    digit mode is added where that leaves none: the widest byte digits with the terms that cover q (at most 64 bits of shift)."""
    out = [(t, w, bal) for t, w in L.ks_pairs(q) for bal in (False, True) if w <= (8 if bal else 7)]
    for bal in (False, True):
        if not any(p[2] == bal and p[1] >= 4 for p in out):
            w = min(8 if bal else 7, q.bit_length() - 1)
            out.append((min(-(-q.bit_length() // w), 63 // w + 1), w, bal))
    return out


ROWS, COLS, CHUNK = 64, 64, 512                     # a workgroup's tile and the slots per pass of its digit image (checked against the stepping's)


def edge_cases(q, full=True):
    """(batch, n_in, n_out, terms, w, balanced) around every edge of the tile code, one dimension at a time from a small base
    (the statement in Python integers costs batch * K * columns products): batches 1, tile - 1, tile, tile + 1 and one past
    two tiles; n_out + 1 of 2 (n_out >= 1: the smallest), column tile - 1, column tile + 1 and one past a workgroup's slab; K =
    n_in * terms of 1, K step - 1, K step + 1 (terms = 1 gives the exact counts) and an odd count past two passes of the image;
    then every byte-wide (terms, w) pair of the modulus at a shape ragged on all three sides.  full=False: the pairs' shapes and
    one case per dimension."""
    out = []
    for bal in (False, True):
        w1 = min(8 if bal else 7, q.bit_length() - 1)
        for batch in ((1, ROWS - 1, ROWS, ROWS + 1, 2 * ROWS + 1) if full else (ROWS + 1,)):
            out.append((batch, K_STEP + 1, 1, 1, w1, bal))
        for cols in ((2, COL_TILE - 1, COL_TILE + 1, COLS + 1) if full else (COLS + 1,)):
            out.append((3, K_STEP - 1, cols - 1, 1, w1, bal))
        for slots in ((1, K_STEP - 1, K_STEP + 1, 2 * CHUNK + 5) if full else (2 * CHUNK + 5,)):
            out.append((3, slots, COL_TILE, 1, w1, bal))
    for terms, w, bal in byte_pairs(q):
        out.append((COL_TILE + 1, -(-(K_STEP + 1) // terms), COL_TILE + 1, terms, w, bal))
    return [c for i, c in enumerate(out) if c not in out[:i]]


FLUSH_Q = L.WORD_SIZE[1]                             # 4294962689: the word 0x7F7F7F80 is below it, 5 limbs
FLUSH_N_IN, FLUSH_TERMS, FLUSH_W, FLUSH_COLS = 32784, 4, 8, 17


def flush_case(rows=16):
    """131,136 products of (-128) * (-128) in every low-limb sum: input words 0x7F7F7F80 (every balanced digit of base 2^8 is
    -128), key words whose two low limbs are -128 (centred residue -128 - 128 * 256), 17 columns -> (lwe, ksk, want).  The
    statement in closed form: every term is 128 * 32896, the body is the word itself."""
    q = FLUSH_Q
    assert L.signed_digits(0x7F7F7F80, q, FLUSH_TERMS, FLUSH_W, True) == [-128] * 4
    assert limbs_of(q - 128 - 128 * 256, q, limb_count(q))[:3] == [-128, -128, 0]
    lwe = np.full((rows, FLUSH_N_IN + 1), 0x7F7F7F80, dtype=np.uint64)
    ksk = np.full((FLUSH_N_IN, FLUSH_TERMS, FLUSH_COLS), q - 128 - 128 * 256, dtype=np.uint64)
    ksk[:, :, 3] = 0                                  # a column of zeros and one of ones among them
    ksk[:, :, 5] = 1
    products = FLUSH_N_IN * FLUSH_TERMS
    assert products == 131136 and products * 2 ** 14 > 2 ** 31 - 1
    want = np.full((rows, FLUSH_COLS), products * 128 * 32896 % q, dtype=np.uint64)
    want[:, 3] = 0
    want[:, 5] = (-128 * products) % q
    want[:, -1] = (int(want[0, -1]) + 0x7F7F7F80) % q
    return lwe, ksk, want


# ---- the stepping's library ---------------------------------------------------------------------------
class EmuLweMfma:
    """The entry points of tests/emu_lwe_mfma/emu_lwe_mfma.cpp in tests/emu_lwe_mfma/_build/libemu_lwe_mfma.so (brought up to date first)."""

    def __init__(self):
        _make("tests/emu_lwe_mfma")
        E = self.lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu_lwe_mfma", "_build", "libemu_lwe_mfma.so"))
        vp, u32, u64, sz, ci = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
        tail = [ctypes.POINTER(ci), ctypes.c_char_p, sz]
        E.emu_lwe_mfma_geometry.argtypes = [ci]; E.emu_lwe_mfma_geometry.restype = u32
        E.emu_lwe_mfma_limbs.argtypes = [u64]; E.emu_lwe_mfma_limbs.restype = u32
        E.emu_lwe_mfma_a_frag_offset.argtypes = [u32, u32, u32]; E.emu_lwe_mfma_a_frag_offset.restype = u32
        E.emu_lwe_mfma_step.argtypes = [vp, vp, vp]; E.emu_lwe_mfma_step.restype = None
        E.emu_lwe_ksk_prepared_bytes.argtypes = [u64, sz, sz, sz, ctypes.POINTER(sz)]
        E.emu_lwe_ksk_prepare.argtypes = [u64, P64, vp, sz, sz, sz]
        E.emu_lwe_keyswitch_prepared.argtypes = [u64, P64, vp, P64, sz, sz, sz, sz, u32, u32]
        E.emu_lwe_ksk_prepared_bytes_api_check.argtypes = [u32, ci, ci, ci, u64, sz, sz, sz, vp] + tail
        E.emu_lwe_ksk_prepare_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, sz, sz, sz] + tail
        E.emu_lwe_keyswitch_prepared_api_check.argtypes = [u32, ci, ci, ci, u64, vp, vp, vp, sz, sz, sz, sz, u32, u32] + tail
        g = [int(E.emu_lwe_mfma_geometry(i)) for i in range(7)]
        self.ROWS, self.COLS, self.K_STEP, self.CHUNK, self.COL_TILE, self.FLUSH_PRODUCTS, self.IMAGE = g

    def limbs(self, q):
        return int(self.lib.emu_lwe_mfma_limbs(q))

    def step(self, a, b, c):
        a, b = np.ascontiguousarray(a, dtype=np.int8), np.ascontiguousarray(b, dtype=np.int8)
        out = np.ascontiguousarray(c, dtype=np.int32).copy()
        assert a.shape == b.shape == (64, 16) and out.shape == (64, 4)
        self.lib.emu_lwe_mfma_step(a.ctypes.data, b.ctypes.data, out.ctypes.data)
        return out

    def bytes(self, q, n_in, n_out, terms):
        size = ctypes.c_size_t(0)
        rc = self.lib.emu_lwe_ksk_prepared_bytes(q, n_in, n_out, terms, ctypes.byref(size))
        assert rc == 0, rc
        return int(size.value)

    @staticmethod
    def _aligned(count, fill):
        """A buffer of `count` bytes at a 16-byte boundary with GUARD_WORDS * 8 guard bytes on either side -> (whole, view)."""
        pad = L.GUARD_WORDS * 8
        raw = np.full(count + 2 * pad + 16, fill, dtype=np.uint8)
        start = pad + (-(raw.ctypes.data + pad)) % 16
        return raw, raw[start:start + count], start

    def prepare(self, q, ksk):
        """-> (the prepared key as uint8, the guard bytes around it are intact)."""
        ksk = np.ascontiguousarray(ksk, dtype=np.uint64)
        n_in, terms, n_out = ksk.shape[0], ksk.shape[1], ksk.shape[2] - 1
        size = self.bytes(q, n_in, n_out, terms)
        raw, view, start = self._aligned(size, 0xA5)
        rc = self.lib.emu_lwe_ksk_prepare(q, p64(ksk), view.ctypes.data, n_in, n_out, terms)
        assert rc == 0, rc
        return view.copy(), bool((raw[:start] == 0xA5).all() and (raw[start + size:] == 0xA5).all())

    def keyswitch(self, q, lwe, ksk, terms, w, balanced, kprep=None):
        """-> (out (batch, n_out + 1), the guards around it are intact); the key is prepared by the stepping unless given."""
        lwe, ksk = np.ascontiguousarray(lwe, dtype=np.uint64), np.ascontiguousarray(ksk, dtype=np.uint64)
        batch, n_in, n_out = lwe.shape[0], lwe.shape[1] - 1, ksk.shape[2] - 1
        assert ksk.shape == (n_in, terms, n_out + 1)
        if kprep is None:
            kprep = self.prepare(q, ksk)[0]
        _, key, _ = self._aligned(kprep.size, 0)
        key[:] = kprep
        buf, out = L.guarded((batch, n_out + 1), np.uint64)
        rc = self.lib.emu_lwe_keyswitch_prepared(q, p64(lwe), key.ctypes.data, out.ctypes.data_as(P64), batch, n_in, n_out, terms, w, int(balanced))
        assert rc == 0, rc
        return out.copy(), L.guards_intact(buf)

    def check(self, which, view, *args):
        """The argument list of entry point `which` ("bytes", "prepare", "keyswitch") on the plan view (n, elem_bytes, has_fused,
        omega_only, q) -> (status, text, goes on)."""
        entry = {"bytes": self.lib.emu_lwe_ksk_prepared_bytes_api_check, "prepare": self.lib.emu_lwe_ksk_prepare_api_check,
                 "keyswitch": self.lib.emu_lwe_keyswitch_prepared_api_check}[which]
        return emu_library.api_check(entry, *view, *args)


@functools.lru_cache(maxsize=None)
def emu_lwe_mfma():
    return EmuLweMfma()


@functools.lru_cache(maxsize=None)
def stepped_flush_key():
    """The flush case's prepared key by the stepping, once per process (read only)."""
    _, ksk, _ = flush_case(1)
    kprep = emu_lwe_mfma().prepare(FLUSH_Q, ksk)[0]
    kprep.setflags(write=False)
    return kprep
