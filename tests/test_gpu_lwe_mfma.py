"""GPU tests of the matrix-core key switch (tn_lwe_ksk_prepare_dev, tn_lwe_keyswitch_prepared_dev; Plan.lwe_ksk_prepare,
Plan.lwe_keyswitch_prepared).  First the lane -> element map of ONE int8 matrix step on the hardware against the host loop that
the CPU stepping is built on (tests/mfmaprobe); then the prepared key byte for byte against the stepping, the key switch word for
word against tn_lwe_keyswitch_dev, the statement in Python integers (tests/lwe_cases.py) and the stepping, with guard words around
every output; the fold of the 32-bit sums; a side stream and one captured graph replayed on rewritten inputs; and the refused rows
through the C ABI."""
import ctypes
import os

import numpy as np
import pytest

import lwe_cases as L
import lwe_mfma_cases as M
from chosen_rows import psi_of
from conftest import ROOT, _make
from lwe_cases import Q23, Q60, Q62, WORD_SIZE
from test_gpu_lwe import dev_words, guarded_out, host, intact

pytestmark = pytest.mark.gpu
N = 256
EINVAL, EUNSUPPORTED = 6, 7


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def emu():
    return M.emu_lwe_mfma()


@pytest.fixture(scope="module")
def probe(eng):
    eng.load_library()                                   # torch's HIP runtime first, as for libtinyntt.so
    _make("tests/mfmaprobe")
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "mfmaprobe", "_build", "libmfmaprobe.so"))
    lib.mfmaprobe_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def step(a, b, c):
        a, b = np.ascontiguousarray(a, dtype=np.int8), np.ascontiguousarray(b, dtype=np.int8)
        out = np.ascontiguousarray(c, dtype=np.int32).copy()
        assert a.shape == b.shape == (64, 16) and out.shape == (64, 4)
        rc = lib.mfmaprobe_step(a.ctypes.data, b.ctypes.data, out.ctypes.data)
        assert rc == 0, rc
        return out
    return step


def test_a_lane_map_of_one_matrix_step(probe, emu):
    """(a) v_mfma_i32_16x16x64_i8 against lwe_mfma_core.h's host loop, bit for bit: every one-hot A element against the one-hot B
    element of its k (64 k x a row and a column that differ, the column moving with k: pins the A, B and C/D maps), a one-hot pair
    whose k differ (no product), random asymmetric bytes with -128 and 127, all from a non-zero accumulator."""
    rng = np.random.default_rng(17)
    for k in range(64):
        row, col = (5 * k + 3) % 16, (7 * k + 1) % 16
        a = np.zeros((64, 16), dtype=np.int8); b = np.zeros((64, 16), dtype=np.int8)
        a[row + 16 * (k // 16), k % 16] = -128
        b[col + 16 * (k // 16), k % 16] = 127 if k % 2 else -128
        c = rng.integers(-1000, 1000, size=(64, 4), dtype=np.int32)
        want = c.copy()
        want[col + 16 * (row // 4), row % 4] += -128 * (127 if k % 2 else -128)
        got = probe(a, b, c)
        assert np.array_equal(got, want), (k, row, col, np.argwhere(got != c).tolist())
        assert np.array_equal(got, emu.step(a, b, c))
    a = np.zeros((64, 16), dtype=np.int8); b = np.zeros((64, 16), dtype=np.int8)
    a[2, 3], b[2, 4] = 77, 55                            # k = 3 against k = 4: nothing to add
    c = rng.integers(-1000, 1000, size=(64, 4), dtype=np.int32)
    assert np.array_equal(probe(a, b, c), c)
    for _ in range(3):
        a = rng.integers(-128, 128, size=(64, 16), dtype=np.int8); b = rng.integers(-128, 128, size=(64, 16), dtype=np.int8)
        a[0, 0], a[1, 1], b[0, 0], b[2, 3] = -128, 127, -128, 127
        c = rng.integers(-2 ** 20, 2 ** 20, size=(64, 4), dtype=np.int32)
        got = probe(a, b, c)
        assert np.array_equal(got, emu.step(a, b, c)) and np.array_equal(got, M.matrix_step(a, b, c))
    a = np.full((64, 16), -128, dtype=np.int8)           # the largest sum of one step: 64 * 2^14
    assert np.array_equal(probe(a, a, np.zeros((64, 4), dtype=np.int32)), np.full((64, 4), 64 * 2 ** 14, dtype=np.int32))


def prepare_guarded(plan, lib, dk, n_in, n_out, terms):
    """tn_lwe_ksk_prepare_dev into a buffer between guard bytes -> (the key's bytes as uint8, guards intact)."""
    import torch
    size, pad = plan.lwe_ksk_prepared_bytes(n_in, n_out, terms), L.GUARD_WORDS * 8
    buf = torch.full((size + 2 * pad,), 0x5A, dtype=torch.uint8, device=dk.device)
    st = lib.tn_lwe_ksk_prepare_dev(plan._h, dk.data_ptr(), buf.data_ptr() + pad, n_in, n_out, terms, plan._stream_ptr(None))
    assert st == 0, lib.tn_last_error().decode()
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return h[pad:pad + size], bool((h[:pad] == 0x5A).all() and (h[pad + size:] == 0x5A).all())


@pytest.mark.parametrize("q", [Q23, Q60], ids=["q23", "q60"])
def test_b_prepared_key_is_the_stepping_s_byte_for_byte(eng, emu, q):
    plan = eng.get_plan(N, q, psi_of(N, q))
    lib = eng.load_library()
    for n_in, terms, n_out in ((1, 1, 1), (13, 5, 16), (3, 43, 64), (40, 4, 300)):
        ksk = L.any_words(np.random.default_rng(n_in), q, (n_in, terms, n_out + 1))
        ksk.reshape(-1)[:2] = (q // 2, q // 2 + 1)
        got, ok = prepare_guarded(plan, lib, dev_words(plan, ksk), n_in, n_out, terms)
        want, _ = emu.prepare(q, ksk)
        assert ok and got.size == M.prepared_bytes(q, n_in, n_out, terms)
        assert np.array_equal(got, want), (n_in, terms, n_out)
        assert np.array_equal(plan.lwe_ksk_prepare(ksk, terms).tensor.cpu().numpy().view(np.uint8), want)      # host values in


def check_case(plan, emu, q, case, stepped=True):
    batch, n_in, n_out, terms, w, balanced = case
    lwe, ksk, want = L.ks_reference(q, n_in, n_out, terms, w, balanced, batch)
    dk, dl = dev_words(plan, ksk).reshape(n_in, terms, n_out + 1), dev_words(plan, lwe)
    key = plan.lwe_ksk_prepare(dk, terms)
    assert (key.n_in, key.n_out, key.terms) == (n_in, n_out, terms)
    buf, out, guard = guarded_out(plan, (batch, n_out + 1))
    plan.lwe_keyswitch_prepared(dl, key, w, balanced, out=out)
    got = host(out)
    assert intact(buf, guard), case
    assert np.array_equal(got, want), case
    assert np.array_equal(got, host(plan.lwe_keyswitch(dl, dk, n_out, terms, w, balanced))), case
    if stepped:
        assert np.array_equal(got, emu.keyswitch(q, lwe, ksk, terms, w, balanced)[0]), case


@pytest.mark.parametrize("q", [Q23, Q60], ids=["q23", "q60"])
def test_c_keyswitch_at_every_edge_of_the_tile_code(eng, emu, q):
    """(c) the edge shapes of tests/test_lwe_mfma_emu.py, both digit modes: tn_lwe_keyswitch_dev, the statement and the stepping."""
    plan = eng.get_plan(N, q, psi_of(N, q))
    for case in M.edge_cases(q):
        check_case(plan, emu, q, case)


@pytest.mark.parametrize("q", WORD_SIZE + (Q62,), ids=[f"q{q}" for q in WORD_SIZE + (Q62,)])
def test_c_word_size_moduli_and_q62(eng, emu, q):
    plan = eng.get_plan(N, q, psi_of(N, q))
    for case in M.edge_cases(q, full=False):
        check_case(plan, emu, q, case)


def test_c_general_and_omega_only_plans_and_host_arrays(eng, emu):
    """An even composite modulus on a general plan, an omega-only plan; host arrays in, host arrays out, one ciphertext in, one out."""
    general = eng.get_general_plan(N, L.EVEN_COMPOSITE, 3)
    omega = eng.get_omega_plan(N, Q60, pow(psi_of(N, Q60), 2, Q60))
    for plan in (general, omega):
        q = plan.q
        for case in M.edge_cases(q, full=False):
            check_case(plan, emu, q, case, stepped=False)
        batch, n_in, n_out, terms, w, balanced = M.edge_cases(q, full=False)[-1]
        lwe, ksk, want = L.ks_reference(q, n_in, n_out, terms, w, balanced, batch)
        key = plan.lwe_ksk_prepare(ksk % np.uint64(q), terms)
        got = plan.lwe_keyswitch_prepared(lwe % np.uint64(q), key, w, balanced)
        assert isinstance(got, np.ndarray) and np.array_equal(got, want)
        one = plan.lwe_keyswitch_prepared(lwe[0] % np.uint64(q), key, w, balanced)
        assert isinstance(one, np.ndarray) and one.shape == (n_out + 1,) and np.array_equal(one, want[0])


def test_d_fold_keeps_sums_past_2_31_exact(eng, emu):
    """(d) the flush case of tests/test_lwe_mfma_emu.py on the device: 131,136 products of 2^14 in every low-limb sum, one launch."""
    q = M.FLUSH_Q
    plan = eng.get_plan(N, q, psi_of(N, q))
    lwe, ksk, want = M.flush_case(16)
    key = plan.lwe_ksk_prepare(dev_words(plan, ksk).reshape(ksk.shape), M.FLUSH_TERMS)
    assert np.array_equal(key.tensor.cpu().numpy().view(np.uint8), M.stepped_flush_key())
    buf, out, guard = guarded_out(plan, want.shape)
    plan.lwe_keyswitch_prepared(dev_words(plan, lwe), key, M.FLUSH_W, True, out=out)
    assert intact(buf, guard) and np.array_equal(host(out), want)
    assert np.array_equal(host(plan.lwe_keyswitch(dev_words(plan, lwe), dev_words(plan, ksk), M.FLUSH_COLS - 1, M.FLUSH_TERMS, M.FLUSH_W, True)), want)


def run_on_side_stream_and_graph(fn, inputs, fresh, out, refs):
    """fn(stream) launches into `out` from `inputs`; fresh[k] are other contents of the inputs and refs[k] the outputs expected
    for them (refs[0]: for the inputs as they are).  A launch on a side stream, then ONE captured graph replayed after the input
    buffer is rewritten (tests/test_gpu_lwe.py's pattern)."""
    import torch
    s1 = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        fn(s1)                                    # also the warm-up outside the capture
    s1.synchronize()
    assert torch.equal(out, refs[0])
    graph = torch.cuda.CUDAGraph(); out.zero_(); torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s1):
        fn(s1)
    for rep in (1, 2):
        out.zero_(); inputs.copy_(fresh[rep]); torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, refs[rep]), rep


def test_e_side_stream_and_captured_graph(eng):
    import torch
    q = Q60
    plan = eng.get_plan(N, q, psi_of(N, q))
    rng = np.random.default_rng(11)
    n_in, n_out, terms, w = 33, 80, 8, 8
    lwe, ksk, want = L.ks_reference(q, n_in, n_out, terms, w, True, M.ROWS + 1)
    dk = dev_words(plan, ksk).reshape(ksk.shape)
    # the key switch: the lwe rows are rewritten between replays
    key = plan.lwe_ksk_prepare(dk, terms)
    sets = [dev_words(plan, lwe)] + [dev_words(plan, L.any_words(rng, q, lwe.shape)) for _ in range(2)]
    refs = [plan.lwe_keyswitch(x, dk, n_out, terms, w, True) for x in sets]
    assert np.array_equal(host(refs[0]), want) and not torch.equal(refs[1], refs[2])
    x, out = sets[0].clone(), torch.zeros_like(refs[0])
    run_on_side_stream_and_graph(lambda s: plan.lwe_keyswitch_prepared(x, key, w, True, out=out, stream=s), x, sets, out, refs)
    # the preparation: the plain key is rewritten between replays
    lib = eng.load_library()
    keys = [dk] + [dev_words(plan, L.any_words(rng, q, ksk.shape)).reshape(ksk.shape) for _ in range(2)]
    refs = [plan.lwe_ksk_prepare(k, terms).tensor for k in keys]
    assert not torch.equal(refs[1], refs[2])
    k, out = keys[0].clone(), torch.zeros_like(refs[0])

    def prepare(s):
        st = lib.tn_lwe_ksk_prepare_dev(plan._h, k.data_ptr(), out.data_ptr(), n_in, n_out, terms, plan._stream_ptr(s))
        assert st == 0, lib.tn_last_error().decode()
    run_on_side_stream_and_graph(prepare, k, keys, out, refs)


def test_f_refused_rows_write_nothing(eng):
    """(f) unsigned base_log 8, balanced base_log 9, a kprep off its alignment and batch 0 through the C ABI; a short kprep and a key
    prepared on another plan from Python (the C call has no size of kprep to look at: include/tinyntt.h).  Each returns its status
    and text, and out keeps its guard pattern."""
    import torch
    q = Q23
    plan, other = eng.get_plan(N, q, psi_of(N, q)), eng.get_plan(N, WORD_SIZE[0], psi_of(N, WORD_SIZE[0]))
    lib = eng.load_library()
    n_in, n_out, terms = 8, 5, 2
    lwe, ksk, _ = L.ks_reference(q, n_in, n_out, terms, 7, False, 3)
    dl, key = dev_words(plan, lwe), plan.lwe_ksk_prepare(ksk, terms)
    buf, out, guard = guarded_out(plan, (3, n_out + 1))
    out.fill_(guard)
    stream = plan._stream_ptr(None)

    def call(kprep, batch, w, flags):
        st = lib.tn_lwe_keyswitch_prepared_dev(plan._h, dl.data_ptr(), kprep, out.data_ptr(), batch, n_in, n_out, terms, w, flags, stream)
        return st, lib.tn_last_error().decode() if st else ""
    name = "tn_lwe_keyswitch_prepared_dev: "
    st, text = call(key.tensor.data_ptr(), 3, 8, 0)
    assert st == EUNSUPPORTED and text.startswith(name + "digits wider than a signed byte") and "tn_lwe_keyswitch_dev is the route" in text
    st, text = call(key.tensor.data_ptr(), 3, 9, 1)
    assert st == EUNSUPPORTED and "tn_lwe_keyswitch_dev is the route" in text
    assert call(key.tensor.data_ptr() + 8, 3, 7, 0) == (EINVAL, name + "kprep must be aligned to 16 bytes")
    assert call(None, 0, 7, 0) == (0, "")
    size = ctypes.c_size_t(0)
    assert lib.tn_lwe_ksk_prepared_bytes(plan._h, n_in, n_out, terms, ctypes.byref(size)) == 0 and size.value == key.tensor.numel() == 3 * 1024
    assert lib.tn_lwe_ksk_prepared_bytes(plan._h, n_in, n_out, 65, ctypes.byref(size)) == EINVAL
    short = eng.PreparedLweKey(plan, key.tensor[:-16], n_in, n_out, terms)
    with pytest.raises(eng.TinyNttError, match="shorter than tn_lwe_ksk_prepared_bytes") as e:
        plan.lwe_keyswitch_prepared(dl, short, 7, out=out)
    assert e.value.status == EINVAL
    with pytest.raises(eng.TinyNttError, match="belongs to another plan") as e:
        plan.lwe_keyswitch_prepared(dl, other.lwe_ksk_prepare(ksk, terms), 7, out=out)
    assert e.value.status == EINVAL
    with pytest.raises(TypeError):
        plan.lwe_keyswitch_prepared(dl, key.tensor, 7, out=out)
    with pytest.raises(eng.TinyNttError, match="signed byte"):
        plan.lwe_keyswitch_prepared(dl, key, 8, out=out)
    torch.cuda.synchronize()
    assert bool((buf == guard).all())
    plan.lwe_keyswitch_prepared(dl, key, 7, out=out)       # ... and the same call with byte-wide digits writes
    assert intact(buf, guard) and np.array_equal(host(out), L.keyswitch(lwe, ksk, q, terms, 7, False))
