"""Plan.bootstrap end to end on the GPU: a toy TFHE scheme written here with numpy and Python integers (n = 256, LWE dimension
16, binary secrets, message space p = 4 with a padding bit, a random table f, batch 8 with each message twice) is bootstrapped
by the library's calls alone (modulus switch, monomial product, blind rotation, sample extraction, key switch), and every output
decrypts to f(m).  Before that the test asserts a worst-case bound, not a statistical one, on the output's phase error and that
it lies below the slot margin q / 4p, so it cannot flake; then that one_launch=True and False give the same bits, and that the
five steps written out by hand give the bits of Plan.bootstrap.

Conventions (include/tinyntt.h): LWE phase b + <a, s>; RLWE phase c0 + c1 z.  The keys follow the library's layouts: RGSW row
[o][i][j] of step k is component o of an encryption of zero plus s_k B^j on component i; ksk[i][j] is an LWE encryption of
z_i B^j.  The constant coefficient of X^rho tv is tv[0], -tv[n - rho], tv[2n - rho] for rho = 0, 0 < rho <= n, rho > n, so
tv[j] = +D f(0) for j < 32 and -D f(slot of n - j) above, D = q / 2p, slots 2n / 2p = 64 exponents wide.

Case A (q = 8380417, no noise, bootstrap key balanced w = 8 x 3 terms, key-switch key unsigned w = 4 x 6 terms).  The balanced
digits are exact for every word but those whose last carry is dropped: words x in (127 (1 + 2^8 + 2^16), q), 0.29 % of the
residues, recompose to x - 2^24 = x - 16382 mod q.  The test counts them in the accumulators of the hand-written route, step by
step, and adds their exact worst case to the bound it asserts: a word of component 0 moves one coefficient of the phase by 16382,
a word of component 1 moves every coefficient by at most 16382 (the secret is binary), only in steps whose key bit is 1.
Case B (q = 2^60 - 2^14 + 1, every encryption with uniform noise |e| <= 4, bootstrap key unsigned w = 20 x 3 terms, key-switch
key unsigned w = 6 x 10 terms): both decompositions cover q, nothing is dropped.  Its bound, 16 * 2 * 3 * 256 * (2^20 - 1) * 4 +
256 * 10 * 63 * 4 + 5 = 103,079,761,925, is below the margin q / 16 = 72,057,594,037,926,912 by a factor of 699,000 = 2^19.4.

Case A's bound is a worst case for THIS instance, not a statistical one and not one known before the run: the dropped words are
counted in the accumulators the library computed from the fixed seed, so the count (and the verdict) is the same on every run, but
another seed gives another count.  The margin q / 16 = 523,776 leaves room for 31 dropped words of component 1 in steps with key
bit 1 (16382 each); about 14 are expected (16 steps, half with key bit 1, 512 words, 0.29 %, counted with the rule above)."""
import numpy as np
import pytest

from chosen_rows import psi_of

pytestmark = pytest.mark.gpu
N, DIM, P, BATCH = 256, 16, 4, 8
SLOT = 2 * N // (2 * P)                      # exponents per message: 64; half a slot is 32
CASES = {
    "A": dict(q=8380417, noise=0, terms=3, w=8, balanced=True, ks_terms=6, ks_w=4),
    "B": dict(q=(1 << 60) - (1 << 14) + 1, noise=4, terms=3, w=20, balanced=False, ks_terms=10, ks_w=6),
}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


def dev(plan, h):
    """Host words -> a device tensor of the plan's words, bit for bit, in the shape of h."""
    import torch
    h = np.ascontiguousarray(np.asarray(h, dtype=np.uint64).astype(plan.dtype))
    return torch.from_numpy(h.view(np.int32 if plan.elem_bytes == 4 else np.int64)).to(f"cuda:{plan.device}")


def centred(x, q):
    x = int(x) % q
    return x - q if x > q // 2 else x


def encode(m, q):
    return (2 * int(m) * q + 2 * P) // (4 * P)                   # round(m q / 2p)


class Toy:
    """Keys, ciphertexts and the table of one case, from one seed."""

    def __init__(self, plan, c, seed):
        self.c, self.q = c, c["q"]
        q, rng = self.q, np.random.default_rng(seed)
        self.noise = lambda shape=None: rng.integers(-c["noise"], c["noise"], size=shape, endpoint=True).astype(object) if c["noise"] else (
            np.zeros(shape, dtype=object) if shape is not None else 0)
        self.s = rng.integers(0, 2, DIM).astype(object)            # the LWE key
        self.z = rng.integers(0, 2, N).astype(object)              # the ring key and, as its coefficients, the big LWE key
        self.f = rng.integers(0, P, P)                             # the table
        self.m = np.array([0, 1, 2, 3, 0, 1, 2, 3])
        # inputs: b = D m + e - <a, s>
        a = rng.integers(0, q, (BATCH, DIM), dtype=np.uint64).astype(object)
        b = (np.array([encode(m, q) for m in self.m], dtype=object) + self.noise(BATCH) - a.dot(self.s)) % q
        self.lwe = np.concatenate([a, b[:, None]], axis=1).astype(np.uint64)
        # test vector
        tv = np.empty(N, dtype=object)
        for j in range(N):
            slot = min((N - j + SLOT // 2) // SLOT, P - 1)
            tv[j] = encode(self.f[0], q) if j < SLOT // 2 else (-encode(self.f[slot], q)) % q
        self.tv = tv.astype(np.uint64)
        # bootstrap key [DIM][o][i][j][n]: (r0, r1) with r0 + r1 z = e, plus s_k B^j on component i
        terms, B = c["terms"], 1 << c["w"]
        r1 = rng.integers(0, q, (DIM, 2, terms, N), dtype=np.uint64)
        zr = np.broadcast_to(self.z.astype(np.uint64), (DIM * 2 * terms, N)).copy()
        r1z = plan.poly_mult(r1.reshape(-1, N), zr).reshape(DIM, 2, terms, N).astype(object)       # key generation: the library's product
        r0 = (self.noise((DIM, 2, terms, N)) - r1z) % q
        bsk = np.empty((DIM, 2, 2, terms, N), dtype=object)
        bsk[:, 0], bsk[:, 1] = r0, r1.astype(object)
        for k in range(DIM):
            for i in range(2):
                for j in range(terms):
                    bsk[k, i, i, j, 0] = (bsk[k, i, i, j, 0] + int(self.s[k]) * B ** j) % q
        self.bsk = bsk.astype(np.uint64).reshape(DIM * 4 * terms, N)
        # key-switch key [N][ks_terms][DIM + 1]: LWE_s(z_i B^j)
        kt, KB = c["ks_terms"], 1 << c["ks_w"]
        ka = rng.integers(0, q, (N, kt, DIM), dtype=np.uint64).astype(object)
        msg = np.array([[int(self.z[i]) * KB ** j for j in range(kt)] for i in range(N)], dtype=object)
        kb = (msg + self.noise((N, kt)) - ka.dot(self.s)) % q
        self.ksk = np.concatenate([ka, kb[:, :, None]], axis=2).astype(np.uint64)

    def phase(self, lwe):
        lwe = np.asarray(lwe).astype(object)
        return (lwe[:, DIM] + lwe[:, :DIM].dot(self.s)) % self.q

    def decrypt(self, lwe):
        return [((2 * P * int(ph) + self.q // 2) // self.q) % (2 * P) for ph in self.phase(lwe)]


def dropped_carry(x, q, terms, w):
    """x (any shape) of canonical words -> True where the balanced digits drop a last carry (recomposition is x - 2^(terms w))."""
    B = np.uint64(1 << w)
    carry = np.zeros(x.shape, dtype=np.uint64)
    for j in range(terms):
        t = ((x >> np.uint64(j * w)) & (B - np.uint64(1))) + carry
        carry = (t >= B // np.uint64(2)).astype(np.uint64)
    return carry.astype(bool)


@pytest.mark.parametrize("case", ["A", "B"])
def test_bootstrap_decrypts_to_the_table(eng, case):
    import torch
    c = CASES[case]
    q = c["q"]
    plan = eng.get_plan(N, q, psi_of(N, q))
    toy = Toy(plan, c, seed=2024 + ord(case))
    assert toy.decrypt(toy.lwe) == toy.m.tolist()
    margin = q // (4 * P)
    B, KB = 1 << c["w"], 1 << c["ks_w"]
    assert c["ks_terms"] * c["ks_w"] >= q.bit_length() and (c["balanced"] or c["terms"] * c["w"] >= q.bit_length())

    # the rounding of the modulus switch: at most (dim + 1) / 2 exponents, plus the input's noise, against half a slot
    in_err = max(abs(centred(int(ph) - encode(m, q), q)) for ph, m in zip(toy.phase(toy.lwe), toy.m))
    assert in_err <= c["noise"]
    assert (DIM + 1) / 2 + in_err * 2 * N / q + 1 < SLOT / 2

    def keys():
        return plan.prepare(toy.bsk), dev(plan, toy.ksk)

    bsk, ksk = keys()
    kw = dict(terms=c["terms"], base_log=c["w"], ks_terms=c["ks_terms"], ks_base_log=c["ks_w"], balanced=c["balanced"])
    dlwe = dev(plan, toy.lwe)

    # the five steps by hand, counting the words whose balanced digits drop a carry (case A) on the way
    exps = plan.lwe_modswitch(dlwe)
    tvs = torch.zeros((BATCH, 2, N), dtype=plan.torch_dtype, device=dlwe.device)
    tvs[:, 0] = plan.to_device(toy.tv.reshape(1, N))[0]
    acc = plan.monomial_mul(tvs, exps[DIM])
    drop = np.zeros(BATCH, dtype=object)
    wrap = ((1 << (c["terms"] * c["w"])) % q) if c["balanced"] else 0
    wrap = min(wrap, q - wrap)
    key_rows = 4 * c["terms"]
    for k in range(DIM):
        if c["balanced"] and int(toy.s[k]):
            x = plan.to_host(plan.monomial_mul(acc, exps[k], minus_one=True).reshape(-1, N)).astype(np.uint64).reshape(BATCH, 2, N)
            hit = dropped_carry(x, q, c["terms"], c["w"])
            drop += wrap * (hit[:, 0].any(axis=1).astype(object) + hit[:, 1].sum(axis=1).astype(object))
        step = eng.PreparedOperand(plan, bsk.tensor[k * key_rows:(k + 1) * key_rows], key_rows)
        acc = plan.poly_cmux_rotate_prepared(acc, exps[k], step, c["terms"], c["w"], c["balanced"])
    big = plan.sample_extract(acc, 0)
    by_hand = plan.lwe_keyswitch(big, ksk, DIM, c["ks_terms"], c["ks_w"])

    # the worst-case bound on the output's phase error, below the slot margin
    per_step = 2 * c["terms"] * N * (B - 1) * c["noise"]
    ks_term = N * c["ks_terms"] * (KB - 1) * c["noise"] + c["noise"]
    rounding = 1                                                       # D f and its negation are rounded to integers
    bound = [DIM * per_step + ks_term + rounding + int(d) for d in drop]
    print(f"case {case}: margin {margin}, bound {max(bound)} (dropped carries {int(max(drop))}), margin / bound {margin / max(bound):.3g}")
    assert max(bound) < margin

    out = {ol: plan.bootstrap(dlwe, bsk, toy.tv, ksk, one_launch=ol, **kw) for ol in (False, True)}
    torch.cuda.synchronize()
    assert torch.equal(out[False], out[True])
    assert torch.equal(out[False], by_hand)
    got = plan.to_host(out[False]).astype(np.uint64)
    want = [int(toy.f[m]) for m in toy.m]
    errs = [abs(centred(int(ph) - encode(fm, q), q)) for ph, fm in zip(toy.phase(got), want)]
    print(f"case {case}: measured phase errors {errs}")
    assert all(e <= b for e, b in zip(errs, bound)), (errs, bound)
    assert toy.decrypt(got) == want
    # host rows in, host rows out
    hout = plan.bootstrap(toy.lwe, bsk, toy.tv, ksk, **kw)
    assert isinstance(hout, np.ndarray) and np.array_equal(hout.astype(np.uint64), got)


def test_bootstrap_on_a_side_stream():
    """stream= a side stream while torch's current stream is another: the method's own torch work (allocations, the zero fill, the
    copy of the test vector) runs under the same stream as the library's calls.  The same bits as on the current stream, from a
    torch stream and from its raw handle; the plan's own stream is refused."""
    import torch
    from tiny_ntt_amd import engine as eng
    c = CASES["A"]
    plan = eng.get_plan(N, c["q"], psi_of(N, c["q"]))
    toy = Toy(plan, c, seed=7)
    bsk, ksk, dlwe, tv = plan.prepare(toy.bsk), dev(plan, toy.ksk), dev(plan, toy.lwe), dev(plan, toy.tv.reshape(1, N))
    kw = dict(terms=c["terms"], base_log=c["w"], ks_terms=c["ks_terms"], ks_base_log=c["ks_w"], balanced=c["balanced"])
    want = plan.bootstrap(dlwe, bsk, tv, ksk, **kw)
    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    for one_launch in (False, True):
        for stream in (s1, s1.cuda_stream):
            assert torch.cuda.current_stream() != s1
            got = plan.bootstrap(dlwe, bsk, tv, ksk, one_launch=one_launch, stream=stream, **kw)
            s1.synchronize()
            assert torch.equal(got, want), (one_launch, stream)
    with pytest.raises(ValueError, match="plan's own stream"):
        plan.bootstrap(dlwe, bsk, tv, ksk, stream="plan", **kw)
    torch.cuda.synchronize()
