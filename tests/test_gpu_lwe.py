"""GPU tests of tn_lwe_modswitch_dev, tn_sample_extract_dev and tn_lwe_keyswitch_dev (Plan.lwe_modswitch, Plan.sample_extract,
Plan.lwe_keyswitch): bit for bit against the statements in Python integers (tests/lwe_cases.py) and against the CPU stepping of
the kernels (tests/emu_lwe/emu_lwe.cpp), with guard words around every output; on a side stream and under one captured graph
replayed on rewritten inputs; and the status order through the C ABI against the argument lists stepped on the CPU."""
import ctypes

import numpy as np
import pytest

import lwe_cases as L
from chosen_rows import psi_of
from lwe_cases import Q23, Q60, WORD_SIZE
from test_lwe_api_emu import EXTRACT, KEYSWITCH, MODSWITCH, NULL, PLAN, WIDE

pytestmark = pytest.mark.gpu
N = 256
MODES = (False, True)


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def emu():
    return L.emu_lwe()


def dev_words(plan, h):
    """Host words of any value -> a device tensor of the plan's words, bit for bit (no reduction)."""
    import torch
    h = np.ascontiguousarray(h, dtype=np.uint64).astype(plan.dtype)
    return torch.from_numpy(h.view(np.int32 if plan.elem_bytes == 4 else np.int64)).to(f"cuda:{plan.device}")


def guarded_out(plan, shape, dtype=None):
    """-> (the whole device buffer filled with the guard word, the view of `shape` between the guards)."""
    import torch
    dtype = dtype or plan.torch_dtype
    count = int(np.prod(shape))
    size = torch.empty((), dtype=dtype).element_size()
    guard = L.GUARD & (2 ** (8 * size) - 1)
    guard -= 2 ** (8 * size) if guard >= 2 ** (8 * size - 1) else 0
    buf = torch.full((count + 2 * L.GUARD_WORDS,), guard, dtype=dtype, device=f"cuda:{plan.device}")
    return buf, buf[L.GUARD_WORDS:L.GUARD_WORDS + count].view(shape), guard


def intact(buf, guard):
    return bool((buf[:L.GUARD_WORDS] == guard).all() and (buf[-L.GUARD_WORDS:] == guard).all())


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).astype(np.uint64)


@pytest.mark.parametrize("q", WORD_SIZE, ids=[f"q{q}" for q in WORD_SIZE])
def test_three_calls_equal_the_statement_and_the_stepping(eng, emu, q):
    """The word-size moduli at n = 256: the modulus switch and the extraction at batch 7 and R + 1; the key switch at (256, 300) and
    (33, 256), batch 7 and R + 1, both digit modes, every (terms, w) pair."""
    import torch
    plan = eng.get_plan(N, q, psi_of(N, q))
    for batch in (7, emu.R + 1):
        for dim in (16, 67):
            lwe = L.modswitch_rows(q, N, batch, dim)
            assert L.has_all_edges(lwe, q, N)
            buf, out, guard = guarded_out(plan, (dim + 1, batch), torch.int32)
            plan.lwe_modswitch(dev_words(plan, lwe), out=out)
            got = host(out).astype(np.uint32)
            assert intact(buf, guard)
            assert np.array_equal(got, L.modswitch(lwe, q, N)) and np.array_equal(got, emu.modswitch(N, q, lwe)[0]), (batch, dim)
        a = L.extract_rows(q, N, batch)
        for index in (0, 1, N // 2, N - 1):
            buf, out, guard = guarded_out(plan, (batch, N + 1))
            plan.sample_extract(dev_words(plan, a.reshape(batch * 2, N)).reshape(batch, 2, N), index, out=out)
            got = host(out)
            assert intact(buf, guard)
            assert np.array_equal(got, L.sample_extract(a, q, index)) and np.array_equal(got, emu.sample_extract(N, q, a, index)[0]), (batch, index)
    for n_in, n_out in ((256, 300), (33, 256)):
        for terms, w in L.ks_pairs(q):
            for balanced in MODES:
                lwe, ksk, want = L.ks_reference(q, n_in, n_out, terms, w, balanced, emu.R + 1)
                dk = dev_words(plan, ksk)
                for batch in (7, emu.R + 1):
                    buf, out, guard = guarded_out(plan, (batch, n_out + 1))
                    plan.lwe_keyswitch(dev_words(plan, lwe[:batch]), dk, n_out, terms, w, balanced, out=out)
                    got = host(out)
                    where = (n_in, n_out, terms, w, balanced, batch)
                    assert intact(buf, guard), where
                    assert np.array_equal(got, want[:batch]), where
                    assert np.array_equal(got, emu.keyswitch(q, lwe[:batch], ksk, terms, w, balanced)[0]), where


@pytest.mark.parametrize("q", [WORD_SIZE[0], WORD_SIZE[1], L.Q62], ids=["32-bit-lanes", "q4294962689", "q62"])
def test_keyswitch_accumulator_worst_case(eng, q):
    """tests/test_lwe_emu.py's worst case on the device: n_in = 4096, the largest digits, key words q - 1."""
    plan = eng.get_plan(N, q, psi_of(N, q))
    lwe, ksk, terms, w = L.worst_case(q)
    for balanced in MODES:
        got = host(plan.lwe_keyswitch(dev_words(plan, lwe), dev_words(plan, ksk), 3, terms, w, balanced))
        assert np.array_equal(got, L.keyswitch(lwe, ksk, q, terms, w, balanced)), balanced


def test_general_and_omega_only_plans_and_host_arrays(eng, emu):
    """The calls need n and q alone: an even composite modulus on a general plan, an omega-only plan; host arrays in, host arrays
    out, one ciphertext in, one out."""
    q = L.EVEN_COMPOSITE
    general = eng.get_general_plan(N, q, 3)
    omega = eng.get_omega_plan(N, Q60, pow(psi_of(N, Q60), 2, Q60))
    for plan in (general, omega):
        qq = plan.q
        lwe = L.modswitch_rows(qq, N, 7, 16)
        got = plan.lwe_modswitch(lwe % np.uint64(qq))
        assert isinstance(got, np.ndarray) and np.array_equal(got, L.modswitch(lwe, qq, N))
        a = L.extract_rows(qq, N, 5)
        got = host(plan.sample_extract(dev_words(plan, a.reshape(10, N)).reshape(5, 2, N), 3))
        assert np.array_equal(got, L.sample_extract(a, qq, 3))
        one = plan.sample_extract(a[1] % np.uint64(qq), 3)
        assert isinstance(one, np.ndarray) and one.shape == (N + 1,) and np.array_equal(one, got[1])
        lwe, ksk, want = L.ks_reference(qq, 33, 256, 3, 7, True, emu.R + 1)
        got = host(plan.lwe_keyswitch(dev_words(plan, lwe), dev_words(plan, ksk), 256, 3, 7, True))
        assert np.array_equal(got, want)
        hk = plan.lwe_keyswitch(lwe[0] % np.uint64(qq), ksk % np.uint64(qq), 256, 3, 7, True)
        assert isinstance(hk, np.ndarray) and hk.shape == (257,) and np.array_equal(hk, want[0])


def run_on_side_stream_and_graph(fn, inputs, fresh, out, refs):
    """fn(stream) launches into `out` from `inputs`; fresh[k] are other contents of the inputs and refs[k] the outputs expected
    for them (refs[0]: for the inputs as they are).  A launch on a side stream, then ONE captured graph (a single kernel node)
    replayed after the input buffer is rewritten."""
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


def test_side_stream_and_captured_graph(eng, emu):
    import torch
    q = Q60
    plan = eng.get_plan(N, q, psi_of(N, q))
    rng = np.random.default_rng(11)
    # modulus switch
    sets = [dev_words(plan, L.any_words(rng, q, (70, 68))) for _ in range(3)]
    refs = [plan.lwe_modswitch(x) for x in sets]
    assert np.array_equal(host(refs[0]).astype(np.uint32), L.modswitch(host(sets[0]), q, N)) and not torch.equal(refs[1], refs[2])
    x, out = sets[0].clone(), torch.zeros_like(refs[0])
    run_on_side_stream_and_graph(lambda s: plan.lwe_modswitch(x, out=out, stream=s), x, sets, out, refs)
    # sample extraction
    sets = [dev_words(plan, L.any_words(rng, q, (18, N))).reshape(9, 2, N) for _ in range(3)]
    refs = [plan.sample_extract(x, 5) for x in sets]
    assert np.array_equal(host(refs[0]), L.sample_extract(host(sets[0]), q, 5)) and not torch.equal(refs[1], refs[2])
    x, out = sets[0].clone(), torch.zeros_like(refs[0])
    run_on_side_stream_and_graph(lambda s: plan.sample_extract(x, 5, out=out, stream=s), x, sets, out, refs)
    # key switch
    lwe, ksk, want = L.ks_reference(q, 33, 256, 3, 20, True, emu.R + 1)
    dk = dev_words(plan, ksk)
    sets = [dev_words(plan, lwe)] + [dev_words(plan, L.any_words(rng, q, lwe.shape)) for _ in range(2)]
    refs = [plan.lwe_keyswitch(x, dk, 256, 3, 20, True) for x in sets]
    assert np.array_equal(host(refs[0]), want) and not torch.equal(refs[1], refs[2])
    x, out = sets[0].clone(), torch.zeros_like(refs[0])
    run_on_side_stream_and_graph(lambda s: plan.lwe_keyswitch(x, dk, 256, 3, 20, True, out=out, stream=s), x, sets, out, refs)


def test_status_order_through_the_c_abi(eng, emu):
    """Every refused row, and every row that launches nothing, of the three argument tables of tests/test_lwe_api_emu.py through the C
    ABI on real plans of the tables' views: the same status and the same text.  (Rows that go on to a launch name made-up
    addresses and stay on the CPU; the parity tests above are the launches.)"""
    import torch
    n, q = PLAN[0], PLAN[4]
    psi4 = next(p for p in (pow(x, (q - 1) // (2 * n), q) for x in range(2, 500)) if pow(p, n, q) == q - 1)
    qw = WIDE[4]
    psiw = next(p for p in (pow(x, (qw - 1) // (2 * n), qw) for x in range(2, 500)) if pow(p, n, qw) == qw - 1)
    plans = {PLAN: eng.get_plan(n, q, psi4), WIDE: eng.get_plan(n, qw, psiw), NULL: None}
    lib = eng.load_library()
    stream = plans[PLAN]._stream_ptr(None)
    ran = 0
    for table, fn in ((MODSWITCH, lib.tn_lwe_modswitch_dev), (EXTRACT, lib.tn_sample_extract_dev)):
        for _, view, x, y, batch, last, status, text, launches in table:
            if launches or view not in plans:
                continue
            st = fn(plans[view]._h if plans[view] else None, x, y, batch, last, stream)
            assert (st, lib.tn_last_error().decode() if st else "") == (status, text)
            ran += 1
    for _, view, lwe, ksk, out, kw, status, text, launches in KEYSWITCH:
        if launches or view not in plans:
            continue
        full = dict(batch=3, n_in=8, n_out=5, terms=2, base_log=4, flags=0)
        full.update(kw)
        st = lib.tn_lwe_keyswitch_dev(plans[view]._h if plans[view] else None, lwe, ksk, out, full["batch"], full["n_in"], full["n_out"], full["terms"],
                                      full["base_log"], full["flags"], stream)
        assert (st, lib.tn_last_error().decode() if st else "") == (status, text)
        ran += 1
    assert ran >= 70                      # (74 rows today)
    # the Python side
    plan = eng.get_plan(N, Q23, psi_of(N, Q23))
    with pytest.raises(eng.TinyNttError, match="index must be below n"):
        plan.sample_extract(np.zeros((1, 2, N), dtype=np.uint32), N)
    with pytest.raises(ValueError):
        plan.sample_extract(np.zeros((1, 3, N), dtype=np.uint32), 0)
    with pytest.raises(ValueError):
        plan.lwe_keyswitch(np.zeros((2, 9), dtype=np.uint32), np.zeros((8, 2, 5), dtype=np.uint32), 5, 2, 4)      # a key of n_out + 1 = 5 words
    with pytest.raises(eng.TinyNttError, match="2\\^base_log < q"):
        plan.lwe_keyswitch(np.zeros((2, 9), dtype=np.uint32), np.zeros((8, 2, 6), dtype=np.uint32), 5, 2, 23)
    x = dev_words(plan, np.zeros((2, 9)))
    with pytest.raises(eng.TinyNttError, match="overlap"):
        plan.lwe_modswitch(x, out=x.view(9, 2))
    torch.cuda.synchronize()
