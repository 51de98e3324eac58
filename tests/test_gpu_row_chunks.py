"""GPU tests of the row hand-out of the persistent fused kernels with chunks of SEVERAL rows (fused_kernels.h: rows come in
chunks of `chunk` consecutive rows; launch_plan.h: plan_rows).  Every family's own tests run rows of 32 KiB and more, a chunk of
one row; here every entry point of tests/row_chunks.py runs at n = 256 / 32-bit lanes and n = 512 / 64-bit lanes, where a chunk
holds 2 to 32 rows, twice:

  * with its rows from the device counter, the last chunk holding a single row;
  * captured into a graph, where a launch gets no counter pair, keeps its chunk and strides over chunks, the last chunk one row
    short.

Every row of both is compared, on the device, with the same entry point run on slabs short enough for the fixed stride of single
rows (the path the families' tests pin to the oracle and the CPU stepping), and a few rows around chunk boundaries and the whole
last chunk with the CPU reference itself.  The output starts as a word no result can hold and has guard rows behind it; every
input has guard rows behind it too.  tests/test_row_chunks_table.py checks without a GPU that these batches cannot stay under the
dynamic threshold."""
import contextlib

import numpy as np
import pytest

from row_chunks import CASES, CASE_IDS, MAX_PER_CU, batches, chosen_rows, device_bytes, plan_rows, row_bytes, shape_params
from test_blindrot_emu import EmuBlindrot
from test_cmux_emu import EmuCmux
from test_dot_emu import sum_mod
from test_extprod_emu import EmuExtprod
from test_gadget2_emu import EmuGadget2
from test_gadget_emu import EmuGadget, gadget_pairs
from test_galoisks_emu import EmuGaloisKs
from test_hat_emu import EmuHat
from test_prepared_emu import EmuPrepared

pytestmark = pytest.mark.gpu
# As device words these are 2^w - 1 and 2^w - 2 of the lane: above every q, and every word a kernel stores is below q.
OUT_SENTINEL, IN_SENTINEL = -1, -2
GALOIS = 5


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def steppers():
    """The CPU steppings, each opened when a case first asks for it."""
    made = {}

    def get(cls):
        if cls not in made:
            made[cls] = cls()
        return made[cls]
    return get


class Guarded:
    """`items` batch items of `per` rows of `cols` words on the device, and `pad` more items behind them that hold `sentinel`: the
    first `items` items are handed to a launch as a contiguous view, and the rest must still hold the sentinel afterwards."""

    def __init__(self, dtype, items, per, cols, pad, sentinel):
        import torch
        self.items, self.per, self.pad, self.sentinel = items, per, pad, sentinel
        self.t = torch.full(((items + pad) * per, cols), sentinel, dtype=dtype, device="cuda:0")

    def rows(self, first, end):
        return self.t[first * self.per:end * self.per]

    def intact_behind(self, items):
        return bool((self.t[items * self.per:] == self.sentinel).all())

    @contextlib.contextmanager
    def shortened(self, items):
        """For a launch of fewer items: the `pad` items behind them hold the sentinel meanwhile."""
        behind = self.rows(items, items + self.pad)
        saved = behind.clone()
        behind.fill_(self.sentinel)
        try:
            yield
        finally:
            behind.copy_(saved)

    def host(self, plan, idx):
        """The rows of the items idx -> (len(idx) * per, cols) uint64."""
        import torch
        sel = torch.tensor(idx, device=self.t.device)
        return plan.to_host(self.rows(0, self.items).reshape(self.items, self.per, -1)[sel].reshape(len(idx) * self.per, -1)).astype(np.uint64)


class Family:
    """One case's inputs for `items` batch items (the words of fill_lcg, guard rows behind them), its entry point on any range
    of them, and its CPU reference on chosen items."""
    out_rows = 1

    def __init__(self, eng, plan, oracle, emu, steppers, case, items, pad):
        self.eng, self.plan, self.oracle, self.emu, self.steppers, self.case = eng, plan, oracle, emu, steppers, case
        self.n, self.q, self.psi = plan.n, plan.q, plan.psi
        self.items, self.pad, self.terms = items, pad, case.terms
        self.w = gadget_pairs(self.q)[0][1]           # digits that cover q in two terms
        self.inputs = []                              # every Guarded a launch reads
        self.key_seed = None
        self.setup()

    # -- buffers --
    def guarded(self, per, cols=None, dtype=None):
        g = Guarded(dtype or self.plan.torch_dtype, self.items, per, cols or self.n, self.pad, IN_SENTINEL)
        self.inputs.append(g)
        return g

    def raw(self, per, seed):
        """Row r of the input = make_poly(seed + 2 r)."""
        g = self.guarded(per)
        self.plan.fill_lcg(self.items * per, seed, 2, out=g.rows(0, self.items))
        return g

    def prepared(self, per, seed):
        """... = the prepared form of make_poly(seed + 2 r)."""
        g = self.guarded(per)
        self.plan.prepare(self.plan.fill_lcg(self.items * per, seed, 2), out=g.rows(0, self.items))
        return g

    def make_key(self, per, seed):
        """A key of `per` prepared rows: one for every item (shared) or one per item."""
        self.key_per, self.key_seed = per, seed
        self.key = self.plan.prepare(self.plan.fill_lcg(per, seed, 2)) if self.case.shared else self.prepared(per, seed)

    def key_of(self, first, end):
        if self.case.shared:
            return self.key
        return self.eng.PreparedOperand(self.plan, self.key.rows(first, end), (end - first) * self.key_per)

    def key_host(self, idx):
        """The prepared rows the items idx are multiplied by: the shared key, or their own keys one after the other."""
        if self.case.shared:
            return self.plan.to_host(self.key.tensor).astype(np.uint64)
        return self.key.host(self.plan, idx)

    def lcg_host(self, seed, per, idx, shared=False):
        """What raw() / make_key() put into the rows of the items idx, before any transform, from the oracle's make_poly."""
        rows = [j if shared else i * per + j for i in idx for j in range(per)]
        return np.stack([self.oracle.make_poly(seed + 2 * r, self.n, self.q) for r in rows])

    def key_lcg_host(self, idx):
        return self.lcg_host(self.key_seed, self.key_per, idx, self.case.shared)

    def items3(self, t, first, end, per):
        return t.rows(first, end).reshape(end - first, per, self.n)

    # -- what a family says --
    def setup(self):
        raise NotImplementedError

    def args(self, first, end):
        """The operands of items [first, end): views and, where needed, new tensors (made outside a capture)."""
        raise NotImplementedError

    def run(self, args, out, stream=None):
        """The entry point into out, ((end - first) * out_rows, n)."""
        raise NotImplementedError

    def cpu(self, idx):
        """-> (len(idx) * out_rows, n) uint64"""
        raise NotImplementedError


class Product(Family):                      # poly_mult, cyclic_poly_mult
    def setup(self):
        self.a, self.b = self.raw(1, 1), self.raw(1, 2)

    def args(self, first, end):
        return self.a.rows(first, end), self.b.rows(first, end)

    def run(self, args, out, stream=None):
        getattr(self.plan, self.case.entry)(*args, variant="fused", out=out, stream=stream)

    def cpu(self, idx):
        ha, hb = self.a.host(self.plan, idx), self.b.host(self.plan, idx)
        if self.case.entry == "poly_mult":
            return self.oracle.poly_mult(ha, hb, self.q, self.psi)
        # python_poly_mult: cg_ntt, cg_ntt, pointwise, cg_intt with omega = psi^2 and no twist (tests/test_emu.py)
        omega, q, out = self.plan.omega, self.q, []
        for x, y in zip(ha, hb):
            X, Y = self.oracle.cg_ntt(x, omega, q), self.oracle.cg_ntt(y, omega, q)
            out.append(self.oracle.cg_intt(np.array([int(u) * int(v) % q for u, v in zip(X, Y)], dtype=np.uint64), omega, q))
        return np.stack(out)


class Transform(Family):                    # ntt_forward, ntt_inverse, twisted_ntt_forward
    def setup(self):
        self.x = self.raw(1, 1)

    def args(self, first, end):
        return (self.x.rows(first, end),)

    def run(self, args, out, stream=None):
        getattr(self.plan, self.case.entry)(args[0], variant="fused", out=out, stream=stream)

    def cpu(self, idx):
        hx, omega = self.x.host(self.plan, idx), self.plan.omega
        if self.case.entry == "ntt_forward":
            return np.stack([self.oracle.cg_ntt(x, omega, self.q) for x in hx])
        if self.case.entry == "ntt_inverse":
            return np.stack([self.oracle.cg_intt(x, omega, self.q) for x in hx])
        return np.stack([self.emu.fused_ntt(self.n, self.q, self.psi, 0, x) for x in hx])      # twist + forward: the stepping


class Prepare(Family):
    def setup(self):
        self.b = self.raw(1, 2)

    def args(self, first, end):
        return (self.b.rows(first, end),)

    def run(self, args, out, stream=None):
        self.plan.prepare(args[0], out=out, stream=stream)

    def cpu(self, idx):
        return self.steppers(EmuPrepared).prepare(self.n, self.q, self.psi, self.b.host(self.plan, idx))


class Unprepare(Family):
    def setup(self):
        self.xhat = self.prepared(1, 1)

    def args(self, first, end):
        return (self.eng.PreparedOperand(self.plan, self.xhat.rows(first, end), end - first),)

    def run(self, args, out, stream=None):
        self.plan.unprepare(args[0], out=out, stream=stream)

    def cpu(self, idx):
        got = self.steppers(EmuHat).unprepare(self.n, self.q, self.psi, self.xhat.host(self.plan, idx))
        assert np.array_equal(got, self.lcg_host(1, 1, idx))          # ... which are the rows that were prepared
        return got


class MultPrepared(Family):
    def setup(self):
        self.a = self.raw(1, 1)
        self.make_key(1, 2)

    def args(self, first, end):
        return self.a.rows(first, end), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_mult_prepared(*args, out=out, stream=stream)

    def cpu(self, idx):
        return self.oracle.poly_mult(self.a.host(self.plan, idx), self.key_lcg_host(idx), self.q, self.psi)


class DotPrepared(Family):
    def setup(self):
        self.a = self.raw(self.terms, 1)
        self.make_key(self.terms, 2)

    def args(self, first, end):
        return self.items3(self.a, first, end, self.terms), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_dot_prepared(*args, out=out, stream=stream)

    def cpu(self, idx):
        products = self.oracle.poly_mult(self.a.host(self.plan, idx), self.key_lcg_host(idx), self.q, self.psi)
        return sum_mod(products.reshape(len(idx), self.terms, self.n), self.q)


class DotHat(Family):
    def setup(self):
        self.ahat = self.prepared(self.terms, 1)
        self.make_key(self.terms, 2)
        self.keep = self.case.mode == "keep_prepared"

    def args(self, first, end):
        return self.eng.PreparedOperand(self.plan, self.ahat.rows(first, end), (end - first) * self.terms), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_dot_hat(*args, self.terms, out=out, stream=stream, keep_prepared=self.keep)

    def cpu(self, idx):
        if self.keep:             # prepared rows out: the stepping, word for word
            return self.steppers(EmuHat).poly_dot_hat(self.n, self.q, self.psi, self.ahat.host(self.plan, idx), self.key_host(idx), self.terms,
                                                      keep_prepared=True)
        products = self.oracle.poly_mult(self.lcg_host(1, self.terms, idx), self.key_lcg_host(idx), self.q, self.psi)
        return sum_mod(products.reshape(len(idx), self.terms, self.n), self.q)


class Gadget(Family):
    def setup(self):
        self.a = self.raw(1, 1)
        self.make_key(self.terms, 2)

    def args(self, first, end):
        return self.a.rows(first, end), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_gadget_dot_prepared(*args, self.terms, self.w, True, out=out, stream=stream)

    def cpu(self, idx):
        return self.steppers(EmuGadget).poly_gadget_dot_prepared(self.n, self.q, self.psi, self.a.host(self.plan, idx), self.key_host(idx), self.terms,
                                                                 self.w, True)


class Gadget2(Family):
    out_rows = 2

    def setup(self):
        self.a = self.raw(1, 1)
        self.make_key(2 * self.terms, 2)

    def args(self, first, end):
        return self.a.rows(first, end), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_gadget_multidot_prepared(*args, 2, self.terms, self.w, True, out=out.reshape(-1, 2, self.n), stream=stream)

    def cpu(self, idx):
        return self.steppers(EmuGadget2).multidot(self.n, self.q, self.psi, self.a.host(self.plan, idx), self.key_host(idx), 2, self.terms, self.w,
                                                  True).reshape(-1, self.n)


class GaloisKs(Family):
    out_rows = 2

    def setup(self):
        self.a = self.raw(2, 1)
        self.make_key(2 * self.terms, 2)

    def args(self, first, end):
        return self.items3(self.a, first, end, 2), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_galois_keyswitch_prepared(args[0], GALOIS, args[1], self.terms, self.w, True, out=out.reshape(-1, 2, self.n), stream=stream)

    def cpu(self, idx):
        ha = self.a.host(self.plan, idx).reshape(len(idx), 2, self.n)
        return self.steppers(EmuGaloisKs).keyswitch(self.n, self.q, self.psi, ha, GALOIS, self.key_host(idx), self.terms, self.w, True).reshape(-1, self.n)


class Extprod(Family):
    out_rows = 2

    def setup(self):
        self.a = self.raw(2, 1)
        self.make_key(2 * 2 * self.terms, 2)

    def args(self, first, end):
        return self.items3(self.a, first, end, 2), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_external_product_prepared(*args, 2, self.terms, self.w, True, out=out.reshape(-1, 2, self.n), stream=stream)

    def cpu(self, idx):
        ha = self.a.host(self.plan, idx).reshape(len(idx), 2, self.n)
        return self.steppers(EmuExtprod).external_product(self.n, self.q, self.psi, ha, self.key_host(idx), self.terms, self.w, True).reshape(-1, self.n)


def random_exponents(shape, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)


def to_device_words(exps):
    import torch
    return torch.from_numpy(np.ascontiguousarray(exps, dtype=np.uint32).view(np.int32)).to("cuda:0")


class Cmux(Family):
    out_rows = 2

    def setup(self):
        import torch
        self.a = self.raw(2, 1)
        self.exps_host = random_exponents(self.items, 3)
        self.exps_host[:4] = (0, self.n, 2 * self.n - 1, 1)
        self.exps = self.guarded(1, 1, torch.int32)
        self.exps.rows(0, self.items).copy_(to_device_words(self.exps_host)[:, None])
        self.make_key(2 * 2 * self.terms, 2)

    def args(self, first, end):
        return self.items3(self.a, first, end, 2), self.exps.rows(first, end), self.key_of(first, end)

    def run(self, args, out, stream=None):
        self.plan.poly_cmux_rotate_prepared(*args, self.terms, self.w, True, out=out.reshape(-1, 2, self.n), stream=stream)

    def cpu(self, idx):
        ha = self.a.host(self.plan, idx).reshape(len(idx), 2, self.n)
        return self.steppers(EmuCmux).rotate(self.n, self.q, self.psi, ha, self.exps_host[idx], self.key_host(idx), self.terms, self.w,
                                             True).reshape(-1, self.n)


class Blindrot(Family):
    out_rows = 2

    def setup(self):
        self.steps = self.case.steps
        self.a = self.raw(2, 1)
        self.exps_host = random_exponents((self.steps, self.items), 4)        # [step][item]: a launch of fewer items has its own tensor
        self.exps_host[0, :4] = (0, self.n, 2 * self.n - 1, 1)
        self.key = self.plan.prepare(self.plan.fill_lcg(self.steps * 4 * self.terms, 2, 2))

    def args(self, first, end):
        return self.items3(self.a, first, end, 2), to_device_words(self.exps_host[:, first:end]), self.key

    def run(self, args, out, stream=None):
        self.plan.poly_blind_rotate_prepared(*args, self.terms, self.w, True, out=out.reshape(-1, 2, self.n), stream=stream)

    def load_accumulator(self, args, out):
        out.copy_(args[0].reshape(-1, self.n))

    def run_in_place(self, args, out, stream=None):
        """out holds the accumulator (load_accumulator) and is rotated in place."""
        acc = out.reshape(-1, 2, self.n)
        got = self.plan.poly_blind_rotate_prepared(acc, args[1], args[2], self.terms, self.w, True, out=acc, stream=stream)
        assert got.data_ptr() == out.data_ptr()

    def cpu(self, idx):
        ha = self.a.host(self.plan, idx).reshape(len(idx), 2, self.n)
        bhat = self.plan.to_host(self.key.tensor).astype(np.uint64)
        return self.steppers(EmuBlindrot).rotate(self.n, self.q, self.psi, ha, self.exps_host[:, idx], bhat, self.terms, self.w, True).reshape(-1, self.n)


FAMILIES = {"poly_mult": Product, "cyclic_poly_mult": Product, "ntt_forward": Transform, "ntt_inverse": Transform, "twisted_ntt_forward": Transform,
            "prepare": Prepare, "unprepare": Unprepare, "poly_mult_prepared": MultPrepared, "poly_dot_prepared": DotPrepared, "poly_dot_hat": DotHat,
            "poly_gadget_dot_prepared": Gadget, "poly_gadget_multidot_prepared": Gadget2, "poly_galois_keyswitch_prepared": GaloisKs,
            "poly_external_product_prepared": Extprod, "poly_cmux_rotate_prepared": Cmux, "poly_blind_rotate_prepared": Blindrot}


def rows_that_differ(got, want, per):
    """The first few batch items whose rows differ, for the message of a failed comparison."""
    bad = (got != want).any(dim=1).reshape(-1, per).any(dim=1)
    return int(bad.sum()), bad.nonzero().reshape(-1)[:8].tolist()


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_chunks_of_several_rows_from_the_counter_and_at_the_fixed_stride(eng, oracle, emu, steppers, case):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b, rb = batches(case, cus), row_bytes(case)
    print(f"{case.entry} {case.shape}: row {rb} B, chunk {b.chunk}, batches {b.dynamic} / {b.captured}, slabs of {b.slab}")
    # not vacuous: both batches are dynamic with a chunk of several rows whatever the occupancy query returns (resident workgroups
    # between one per CU and one per wave slot), neither is a multiple of the chunk, and a slab keeps the fixed stride of single rows
    assert b.chunk >= 2
    for batch in (b.dynamic, b.captured):
        assert batch % b.chunk != 0
        for resident in (cus, MAX_PER_CU * cus):
            assert plan_rows(rb, batch, resident) == (True, b.chunk)
    assert plan_rows(rb, b.slab, cus) == (False, 1)
    torch.cuda.empty_cache()
    free, need = torch.cuda.mem_get_info()[0], device_bytes(case, b)
    if free < need:
        pytest.skip(f"needs ~{need / 2 ** 30:.1f} GiB of free HBM, {free / 2 ** 30:.1f} GiB available")
    n, q, psi, word = shape_params(case.shape)
    plan = eng.get_plan(n, q, psi)
    assert plan.has_fused and plan.elem_bytes == word
    items = max(b.dynamic, b.captured)
    fam = FAMILIES[case.entry](eng, plan, oracle, emu, steppers, case, items, b.chunk)
    per = fam.out_rows
    in_place = case.mode == "in_place"
    launch = fam.run_in_place if in_place else fam.run

    # every row from slabs at the fixed stride of single rows, once, for both launches
    expected = torch.empty((items * per, n), dtype=plan.torch_dtype, device="cuda:0")
    for first in range(0, items, b.slab):
        end = min(first + b.slab, items)
        fam.run(fam.args(first, end), expected[first * per:end * per])
    torch.cuda.synchronize()
    # ... and a few of them from the CPU reference, so that the slabs are not the only witness
    chosen = {batch: chosen_rows(b.chunk, batch) for batch in (b.dynamic, b.captured)}
    idx = sorted(set(chosen[b.dynamic]) | set(chosen[b.captured]))
    want = fam.cpu(idx).reshape(len(idx), per, n)
    want_of = dict(zip(idx, want))

    out = Guarded(plan.torch_dtype, items, per, n, b.chunk, OUT_SENTINEL)

    def arm(args, view):
        out.t.fill_(OUT_SENTINEL)
        if in_place:
            fam.load_accumulator(args, view)
        torch.cuda.synchronize()

    problems = []                             # every launch is checked in full; the test fails at its end with all of them

    def check(batch, what):
        torch.cuda.synchronize()
        got, exp = out.rows(0, batch), expected[:batch * per]
        if not out.intact_behind(batch):
            problems.append((what, batch, "rows past the end of the output were written"))
        if not all(g.intact_behind(batch) for g in fam.inputs):
            problems.append((what, batch, "rows past the end of an input were written"))
        unwritten = (got == OUT_SENTINEL).any(dim=1).reshape(-1, per).any(dim=1)
        if bool(unwritten.any()):
            problems.append((what, batch, "items never written", int(unwritten.sum()), "the first", unwritten.nonzero().reshape(-1)[:8].tolist()))
        if not torch.equal(got, exp):
            problems.append((what, batch, "items differ from the slabs", *rows_that_differ(got, exp, per)))
        sel = chosen[batch]
        host = plan.to_host(got.reshape(batch, per, n)[torch.tensor(sel, device=got.device)]).astype(np.uint64)
        differ = [r for r, row in zip(sel, host) if not np.array_equal(row, want_of[r])]
        if differ:
            problems.append((what, batch, "items differ from the CPU reference", differ))

    # 1. rows from the device counter; the last chunk holds one row
    with contextlib.ExitStack() as stack:
        for g in fam.inputs:
            stack.enter_context(g.shortened(b.dynamic))
        args, view = fam.args(0, b.dynamic), out.rows(0, b.dynamic)
        arm(args, view)
        launch(args, view)
        check(b.dynamic, "dynamic")
        if in_place:                          # ... and the bits of the launch with an output of its own
            apart = Guarded(plan.torch_dtype, b.dynamic, per, n, b.chunk, OUT_SENTINEL)
            fam.run(args, apart.rows(0, b.dynamic))
            torch.cuda.synchronize()
            if not (apart.intact_behind(b.dynamic) and torch.equal(view, apart.rows(0, b.dynamic))):
                problems.append(("dynamic", b.dynamic, "in place differs from the launch with an output of its own"))
            del apart

    # 2. no counter pair: the same call captured into a graph (one kernel node, no parallel branches), replayed twice onto a
    #    re-armed output; the last chunk is one row short
    args, view = fam.args(0, b.captured), out.rows(0, b.captured)
    s1 = torch.cuda.Stream()
    arm(args, view)                           # everything so far ran on the default stream: s1 starts behind it
    with torch.cuda.stream(s1):
        launch(args, view, stream=s1)         # warm-up outside the capture
    s1.synchronize()
    check(b.captured, "warm-up")
    g = torch.cuda.CUDAGraph()
    arm(args, view)
    with torch.cuda.graph(g, stream=s1):
        launch(args, view, stream=s1)
    for rep in range(2):
        arm(args, view)
        with torch.cuda.stream(s1):
            g.replay()
        check(b.captured, f"replay {rep}")
    assert not problems, "\n".join([f"{CASE_IDS[CASES.index(case)]}, chunk {b.chunk}:"] + [" ".join(str(v) for v in p) for p in problems])
