"""Plan.pack_lwes end to end on the GPU: a toy scheme written here with numpy and Python integers (n = 256, a binary ring key z whose
coefficients are the LWE key, groups 3, count in {1, 2, 8, 256}) packs LWE ciphertexts into RLWE ciphertexts with the library's
calls alone (lwe_embed, poly_pack_step_prepared level by level, the trace steps).

Conventions (include/tinyntt.h): LWE phase b + <a, z>; RLWE phase c0 + c1 z.  Level t's key, for g = 2^t + 1, is
K[1][j] = r_j (random), K[0][j] = B^j sigma_g(z) + e_j - r_j z, so K[0][j] + K[1][j] z = B^j sigma_g(z) + e_j: a key from sigma_g(z)
to z in the layout of poly_galois_keyswitch_prepared.  Digits are unsigned and cover q (3 x 8 bits for the 23-bit modulus, 3 x 21
bits for the 60-bit one), so nothing is dropped and a noise-free run is exact.

The factor n.  Every level adds a ciphertext to an automorphism of (nearly) itself, which doubles the coefficients that are kept and
cancels the rest; log2 n levels in all, so the phase of the result is n * sum_j mu_j X^(j n / count), where mu_j is the phase of
LWE ciphertext j.  The library does not remove the factor; the tests state it.

The bound of the noisy case is a worst case derived from the parameters, not a statistical one: with |e| <= eta on every LWE
body and every key row, one automorphism key switch adds at most V = terms * n * (B - 1) * eta to any coefficient (terms products of
a digit row below B with a noise row); a pack level maps a bound E on both inputs to 2 (E + E) + V (the sum and the automorphism
of the difference), a trace step to 2 E + V.  Starting from eta the recursion gives the asserted bound, which the test also
requires to lie below the decoding margin q / 2p minus the rounding slack of the encoding."""
import numpy as np
import pytest

from chosen_rows import psi_of
from test_cmux_emu import TRIVIAL
from test_galois_emu import sigma
from test_gpu_bootstrap import dev
from test_gpu_pack import explicit

pytestmark = pytest.mark.gpu
N, GROUPS, P = 256, 3, 4
COUNTS = (1, 2, 8, 256)
Q23, Q60 = 8380417, (1 << 60) - (1 << 14) + 1
CASES = {"q23_noise_free": (Q23, 0), "q60_noise_free": (Q60, 0), "q60_noisy": (Q60, 4)}


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


class Toy:
    """The ring key, the log2 n automorphism keys and a way to encrypt and decrypt, of one modulus and noise width, from one seed."""

    def __init__(self, eng, q, eta, seed):
        from tiny_ntt_amd import numtheory
        self.q, self.eta = q, eta
        self.plan = plan = eng.get_plan(N, q, psi_of(N, q))
        self.terms, self.w = TRIVIAL[q.bit_length()]
        assert self.terms * self.w >= q.bit_length() and (1 << self.w) < q
        self.rng = rng = np.random.default_rng(seed)
        self.z = rng.integers(0, 2, N).astype(np.uint64)
        self.levels = numtheory.pack_elements(N)
        assert self.levels == [(N >> t, (1 << t) + 1) for t in range(1, 9)]
        rows = []
        for _, g in self.levels:
            r = rng.integers(0, q, (self.terms, N), dtype=np.uint64)
            rz = plan.poly_mult(r, np.broadcast_to(self.z, (self.terms, N)).copy()).astype(object)      # key generation: the library's product
            sz = sigma(self.z, g, q).astype(object)
            k0 = np.array([(sz * (1 << (j * self.w)) + self.noise(N) - rz[j]) % q for j in range(self.terms)], dtype=object)
            rows += [k0.astype(np.uint64), r]
        self.keys = plan.prepare(np.concatenate(rows))                 # [level][2][terms][n]
        assert self.keys.rows == len(self.levels) * 2 * self.terms

    def noise(self, shape):
        if not self.eta:
            return np.zeros(shape, dtype=object)
        return self.rng.integers(-self.eta, self.eta, size=shape, endpoint=True).astype(object)

    def encrypt(self, mu):
        """mu (groups, count) Python integers -> LWE rows (groups, count, n + 1) with phase mu + e."""
        a = self.rng.integers(0, self.q, mu.shape + (N,), dtype=np.uint64)
        b = (mu.astype(object) + self.noise(mu.shape) - a.astype(object).dot(self.z.astype(object))) % self.q
        return np.concatenate([a, b.astype(np.uint64)[..., None]], axis=-1)

    def phase(self, ct):
        """RLWE ciphertexts (rows, 2, n) on the device -> their phases (rows, n), host."""
        import torch
        rows = int(ct.shape[0])
        zs = dev(self.plan, np.broadcast_to(self.z, (rows, N)).copy())
        c1z = self.plan.poly_mult(ct[:, 1].contiguous(), zs).to(torch.int64) + ct[:, 0].to(torch.int64)
        return self.plan.to_host(torch.where(c1z >= self.q, c1z - self.q, c1z).to(self.plan.torch_dtype)).astype(np.uint64)

    def lwe_phase(self, lwe):
        lwe = np.asarray(lwe).astype(object)
        return (lwe[..., N] + lwe[..., :N].dot(self.z.astype(object))) % self.q


@pytest.fixture(scope="module")
def toys(eng):
    made = {}

    def get(name):
        if name not in made:
            q, eta = CASES[name]
            made[name] = Toy(eng, q, eta, 20 + len(made))
        return made[name]
    return get


def packed_want(mu, count, q):
    """n * sum_j mu_j X^(j n / count) mod q: (groups, n) Python integers."""
    want = np.zeros((mu.shape[0], N), dtype=object)
    want[:, np.arange(count) * (N // count)] = (mu.astype(object) * N) % q
    return want


def route_tree(plan, lwe, keys, terms, w):
    """pack_lwes written with the explicit route: the same halves, rotations and elements, every level through
    tests/test_gpu_pack.py's explicit (monomial_mul, torch sums, poly_galois_keyswitch_prepared, the addition)."""
    from tiny_ntt_amd import engine, numtheory
    groups, count = int(lwe.shape[0]), int(lwe.shape[1])
    cur = plan.lwe_embed(lwe.transpose(0, 1).contiguous().reshape(count * groups, N + 1), 0)
    for t, (k, g) in enumerate(numtheory.pack_elements(N), start=1):
        key = engine.PreparedOperand(plan, keys.tensor[(t - 1) * 2 * terms:t * 2 * terms], 2 * terms)
        rows = int(cur.shape[0])
        if rows > groups:
            cur = explicit(plan, cur[:rows // 2], cur[rows // 2:], k, g, key, terms, w, False)
        else:
            cur = explicit(plan, cur, None, 0, g, key, terms, w, False)
    return cur


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", ["q23_noise_free", "q60_noise_free"])
def test_noise_free_packing_is_exact(toys, name, count):
    """Any messages mod q: the decrypted phase is n * sum_j mu_j X^(j n / count) exactly and every other coefficient is 0; the result
    is the route-built tree's, bit for bit; the sample extracted at j n / count has the phase n mu_j."""
    import torch
    toy = toys(name)
    plan, q = toy.plan, toy.q
    mu = toy.rng.integers(0, q, (GROUPS, count), dtype=np.uint64)
    lwe = dev(plan, toy.encrypt(mu))
    assert np.array_equal(toy.lwe_phase(plan.to_host(lwe)), mu.astype(object))
    ct = plan.pack_lwes(lwe, toy.keys, toy.terms, toy.w)
    assert ct.shape == (GROUPS, 2, N)
    assert torch.equal(ct, route_tree(plan, lwe, toy.keys, toy.terms, toy.w))
    want = packed_want(mu, count, q)
    phase = toy.phase(ct).astype(object)
    assert np.array_equal(phase, want), (name, count)
    if count < N:
        assert np.count_nonzero(np.delete(phase, np.arange(count) * (N // count), axis=1)) == 0
    for j in sorted({0, count // 2, count - 1}):
        got = toy.lwe_phase(plan.to_host(plan.sample_extract(ct, j * (N // count))))
        assert np.array_equal(got, (mu[:, j].astype(object) * N) % q), (name, count, j)


def error_bound(eta, terms, w, count):
    """The worst case of the module docstring, from the parameters alone."""
    v = terms * N * ((1 << w) - 1) * eta
    e = eta
    packs = count.bit_length() - 1
    for level in range(N.bit_length() - 1):
        e = 4 * e + v if level < packs else 2 * e + v
    return e


@pytest.mark.parametrize("count", COUNTS)
def test_noisy_packing_stays_within_the_worst_case_and_decrypts(toys, count):
    """60-bit modulus, |e| <= 4 on every LWE body and key row; messages m in [0, p) encoded as mu = m * round(q / (n p)), so that
    n mu is m q / p up to a rounding slack below n p / 2 per unit of m: every coefficient of the phase is within the worst-case bound
    of n * sum_j mu_j X^(j n / count), the bound lies below the decoding margin, and sample_extract at j n / count decrypts to m_j."""
    import torch
    toy = toys("q60_noisy")
    plan, q = toy.plan, toy.q
    delta = (2 * q + N * P) // (2 * N * P)                        # round(q / (n p))
    slack = (P - 1) * abs(N * delta * P - q) // P + 1             # |n mu - m q / p| <= m |n delta p - q| / p
    m = toy.rng.integers(0, P, (GROUPS, count))
    mu = (m.astype(object) * delta) % q
    lwe = dev(plan, toy.encrypt(mu))
    bound = error_bound(toy.eta, toy.terms, toy.w, count)
    assert bound + slack < q // (2 * P), (bound, slack)
    ct = plan.pack_lwes(lwe, toy.keys, toy.terms, toy.w)
    assert torch.equal(ct, route_tree(plan, lwe, toy.keys, toy.terms, toy.w))
    diff = (toy.phase(ct).astype(object) - packed_want(mu, count, q)) % q
    worst = max(min(int(d), q - int(d)) for d in diff.ravel())
    print(f"count {count}: worst phase error {worst}, bound {bound}")
    assert worst <= bound, (count, worst, bound)
    for j in sorted({0, count // 2, count - 1}):
        ph = toy.lwe_phase(plan.to_host(plan.sample_extract(ct, j * (N // count))))
        assert [((2 * P * int(x) + q) // (2 * q)) % P for x in ph] == [int(v) for v in m[:, j]], (count, j)


def test_side_stream_orders_the_copy_the_allocations_and_the_launches(toys):
    """pack_lwes on a side stream (count 8: the slot-major copy is a kernel of torch's), twice, while the default stream is kept busy
    with allocations and fills of the same sizes: the method's own torch work runs under the given stream, so both results equal
    the default stream's; a raw stream handle is taken as well, and the plan's own stream is refused."""
    import torch
    toy = toys("q60_noise_free")
    plan = toy.plan
    lwe = dev(plan, toy.encrypt(toy.rng.integers(0, toy.q, (GROUPS, 8), dtype=np.uint64)))
    want = plan.pack_lwes(lwe, toy.keys, toy.terms, toy.w)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got = []
    for stream in (side, side.cuda_stream):
        with torch.cuda.stream(side):
            fresh = lwe.clone()                                            # written on the side stream just before it is read there
        got.append(plan.pack_lwes(fresh, toy.keys, toy.terms, toy.w, stream=stream))
        for _ in range(4):                                                 # the default stream takes and returns blocks meanwhile
            torch.empty((8 * GROUPS, 2, N), dtype=plan.torch_dtype, device=lwe.device).fill_(-1)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    with pytest.raises(ValueError, match="plan's own stream"):
        plan.pack_lwes(lwe, toy.keys, toy.terms, toy.w, stream="plan")


def test_arguments_of_pack_lwes(eng, toys):
    import torch
    toy = toys("q23_noise_free")
    plan = toy.plan
    lwe = dev(plan, toy.encrypt(np.zeros((GROUPS, 4), dtype=np.uint64)))
    with pytest.raises(ValueError):
        plan.pack_lwes(lwe[:, :3].contiguous(), toy.keys, toy.terms, toy.w)                # count 3
    with pytest.raises(ValueError):
        plan.pack_lwes(lwe[:, :, :N].contiguous(), toy.keys, toy.terms, toy.w)             # rows of n words
    with pytest.raises(ValueError):
        plan.pack_lwes(lwe, eng.PreparedOperand(plan, toy.keys.tensor[:2 * toy.terms], 2 * toy.terms), toy.terms, toy.w)      # one level's key
    with pytest.raises(ValueError):
        plan.pack_lwes(plan.to_host(lwe), toy.keys, toy.terms, toy.w)                      # a host array
    torch.cuda.synchronize()
