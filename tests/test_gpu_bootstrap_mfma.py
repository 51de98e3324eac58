"""Plan.bootstrap with a prepared key-switch key (Plan.lwe_ksk_prepare) on the GPU: bit for bit what it returns with the plain
key, on tests/test_gpu_bootstrap.py's toy scheme (n = 256, LWE dimension 16; q = 8380417 with key-switch digits of 4 bits, q =
2^60 - 2^14 + 1 with digits of 6 bits), both one_launch settings, device rows and host rows, also with balanced key-switch digits
of 8 bits; and the outputs still decrypt to the table."""
import numpy as np
import pytest

from chosen_rows import psi_of
from test_gpu_bootstrap import CASES, DIM, N, Toy, dev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ["A", "B"])
def test_bootstrap_with_the_prepared_key_equals_the_plain_key(case):
    import torch
    from tiny_ntt_amd import engine as eng
    c = CASES[case]
    q = c["q"]
    plan = eng.get_plan(N, q, psi_of(N, q))
    toy = Toy(plan, c, seed=31 + ord(case))
    bsk, ksk, dlwe = plan.prepare(toy.bsk), dev(plan, toy.ksk), dev(plan, toy.lwe)
    key = plan.lwe_ksk_prepare(ksk, c["ks_terms"])
    assert (key.n_in, key.n_out, key.terms) == (N, DIM, c["ks_terms"]) and c["ks_w"] <= 7
    kw = dict(terms=c["terms"], base_log=c["w"], ks_terms=c["ks_terms"], ks_base_log=c["ks_w"], balanced=c["balanced"])
    for one_launch in (False, True):
        plain = plan.bootstrap(dlwe, bsk, toy.tv, ksk, one_launch=one_launch, **kw)
        prepared = plan.bootstrap(dlwe, bsk, toy.tv, key, one_launch=one_launch, **kw)
        torch.cuda.synchronize()
        assert torch.equal(plain, prepared), one_launch
    assert toy.decrypt(plan.to_host(prepared).astype(np.uint64)) == [int(toy.f[m]) for m in toy.m]
    hout = plan.bootstrap(toy.lwe, bsk, toy.tv, key, **kw)                  # host rows in, host rows out
    assert isinstance(hout, np.ndarray) and np.array_equal(hout.astype(np.uint64), plan.to_host(prepared).astype(np.uint64))
    # the same key read with balanced digits of 8 bits: not a key switch of this scheme, the same bits from both routes
    kw8 = dict(kw, ks_terms=c["ks_terms"], ks_base_log=8 if (c["ks_terms"] - 1) * 8 < 64 else 7, ks_balanced=True)
    assert torch.equal(plan.bootstrap(dlwe, bsk, toy.tv, ksk, **kw8), plan.bootstrap(dlwe, bsk, toy.tv, key, **kw8))
    # a key of another shape, and digits wider than a byte, are refused
    with pytest.raises(ValueError, match="prepared key of shape"):
        plan.bootstrap(dlwe, bsk, toy.tv, plan.lwe_ksk_prepare(ksk.reshape(N // 2, 2 * c["ks_terms"], DIM + 1), 2 * c["ks_terms"]), **kw)
    if (c["ks_terms"] - 1) * 8 < 64:                                        # (else the gadget rule refuses unsigned digits of 8 bits first)
        with pytest.raises(eng.TinyNttError, match="signed byte"):
            plan.bootstrap(dlwe, bsk, toy.tv, key, **dict(kw, ks_base_log=8))
    torch.cuda.synchronize()
