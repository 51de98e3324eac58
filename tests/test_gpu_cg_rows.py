"""GPU tests of the row loop of the constant-geometry kernel (cg_kernel_impl.h: "Row hand-out" and the loop below it) when a
workgroup runs MORE THAN ONE ROW.  cg_kernel is the only kernel behind every size below n = 256, every general plan and every
omega-only plan, and the rest of the suite runs it there with one row per workgroup: the loop body once, no next-row slot ever
read for a second row.  Every case of tests/cg_rows.py is launched three times:

  1. with its rows from the device counter, in chunks of several rows, the last chunk holding a single row;
  2. captured into a graph (one kernel node) and replayed twice with other inputs: a launch that planned dynamic rows and got no
     counter pair hands out single rows at the fixed stride (CG_ROWS.single_rows_without_slot); the warm-up launch on the side
     stream is live and takes the same batch, one row short of a whole chunk, from the counter;
  3. at the fixed stride of single rows with a batch that makes every workgroup go round the loop.

The same loop runs in all three, so no launch in which a workgroup runs two rows may serve as the reference.  The inputs are
PERIODIC instead: row r of every operand is row (r + shift) mod P of a base block of P rows, and the expected row r is row
(r + shift) mod P of the entry point's output on the base block alone, a launch of P <= CUs rows, one row per workgroup (the path
the rest of the suite pins to the oracle), all P rows of which are compared with the CPU reference here as well.  P is a prime
above 128 that does not divide the CU count (cg_rows.period): it is coprime to every chunk (a power of two), to every grid (at
most 32 workgroups per CU times the CU count) and to their products, and a hand-out error displaces rows by multiples of the
chunk or of grid * chunk, never by a multiple of P: a displaced, skipped or doubled row meets other expected words or the word
the output was filled with.

The output starts as a word no result can hold; it and every input have guard rows of another such word IN FRONT and BEHIND.
After each launch the guards must be intact, the inputs unchanged and every row right; all comparisons run on the device, in
pieces.  tests/test_cg_rows_table.py checks without a GPU that the batches are what they are taken for."""
import numpy as np
import pytest

from cg_rows import (CASES, CASE_IDS, MAX_PER_CU, PRODUCTS, base_rows, batches, device_bytes, period, plan_rows, reference, row_bytes,
                     shape_params)

pytestmark = pytest.mark.gpu
# As device words these are 2^w - 1 and 2^w - 2 of the lane: above every q, and every word a kernel stores is below q.
OUT_SENTINEL, IN_SENTINEL = -1, -2
PIECE_WORDS = 1 << 25           # words per piece of a comparison: its temporaries stay below 1/8 of the smallest operand


@pytest.fixture(scope="module")
def eng():
    import torch
    assert torch.cuda.is_available()
    from tiny_ntt_amd import engine
    return engine


@pytest.fixture(scope="module")
def blocks(oracle):
    """The base block of a shape and the CPU reference of an entry point on it, computed once per module."""
    made = {}

    def get(shape, entry, rows):
        key = (shape, entry, rows)
        if key not in made:
            a = base_rows(shape, rows, 0)
            b = base_rows(shape, rows, 1) if entry in PRODUCTS else None
            made[key] = (a, b, reference(oracle, shape, entry, a, b))
        return made[key]
    return get


def make_plan(eng, shape):
    kind, n, q, psi, omega, word = shape_params(shape)
    plan = eng.get_omega_plan(n, q, omega) if kind == "omega" else eng.get_general_plan(n, q, psi) if kind == "general" else eng.get_plan(n, q, psi)
    assert (plan.n, plan.q, plan.omega, plan.elem_bytes) == (n, q, omega, word)
    assert plan.general == (kind == "general") and plan.omega_only == (kind == "omega")
    return plan


class Guarded:
    """`items` rows of `cols` words on the device between `pad` rows in front and `pad` rows behind, all filled with `sentinel`.
    A launch gets the first `batch` of the rows in the middle as a contiguous view; the rows in front of it and the rows behind
    it (the rest of the middle, then the pad) must still hold the sentinel afterwards."""

    def __init__(self, dtype, items, cols, pad, sentinel):
        import torch
        self.items, self.pad, self.sentinel = items, pad, sentinel
        self.t = torch.full((pad + items + pad, cols), sentinel, dtype=dtype, device="cuda:0")

    def reset(self):
        self.t.fill_(self.sentinel)

    def rows(self, batch):
        assert batch <= self.items
        return self.t[self.pad:self.pad + batch]

    def guards_intact(self, batch):
        reach = max(self.pad, PIECE_WORDS // self.t.shape[1])
        front, behind = self.t[:self.pad], self.t[self.pad + batch:self.pad + batch + reach]
        return bool((front == self.sentinel).all()) and bool((behind == self.sentinel).all())


def fill_periodic(view, block):
    """view[r] = block[r mod P]: the gather, as a broadcast copy of whole periods and a last partial one."""
    P = block.shape[0]
    k, rem = divmod(view.shape[0], P)
    if k:
        view[:k * P].view(k, P, -1).copy_(block.unsqueeze(0).expand(k, P, -1))
    if rem:
        view[k * P:].copy_(block[:rem])


def compare_periodic(view, block, sentinel=None):
    """view[r] against block[r mod P], in pieces of whole periods -> (rows that differ, the first few, rows that hold the
    sentinel in some word, the first few)."""
    import torch
    P, n = block.shape
    step = max(1, PIECE_WORDS // (P * n)) * P
    counts, firsts = [0, 0], [[], []]
    for first in range(0, view.shape[0], step):
        end = min(first + step, view.shape[0])
        k, rem = divmod(end - first, P)
        parts = [(first, view[first:first + k * P].view(k, P, n), block)] if k else []
        if rem:
            parts.append((first + k * P, view[first + k * P:end].view(1, rem, n), block[:rem]))
        for at, v, blk in parts:
            flags = [(v != blk).any(dim=2).reshape(-1)]
            if sentinel is not None:
                flags.append((v == sentinel).any(dim=2).reshape(-1))
            for which, (bad, nbad) in enumerate(zip(flags, torch.stack([f.sum() for f in flags]).tolist())):
                if nbad:
                    counts[which] += nbad
                    if len(firsts[which]) < 8:
                        firsts[which] += (bad.nonzero().reshape(-1)[:8 - len(firsts[which])] + at).tolist()
    return counts[0], firsts[0], counts[1], firsts[1]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_row_loop_from_the_counter_without_a_counter_pair_and_at_the_fixed_stride(eng, blocks, case):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b, rb, P = batches(case, cus), row_bytes(case), period(cus)
    print(f"{case.shape} {case.entry} {case.variant}: row {rb} B, chunk {b.chunk}, batches {b.dynamic} / {b.captured} / {b.fixed}, period {P}")
    # not vacuous: the first two batches are dynamic with a chunk of several rows whatever the occupancy query returns (resident
    # workgroups between one per CU and one per wave slot), neither is a multiple of the chunk, the third keeps the fixed stride
    # of single rows and is longer than any grid; a launch of the base block is one row per workgroup
    assert b.chunk >= 2 and P <= cus < b.fixed and MAX_PER_CU * cus < b.fixed
    for batch in (b.dynamic, b.captured):
        assert batch % b.chunk != 0
        for resident in (cus, MAX_PER_CU * cus):
            assert plan_rows(rb, batch, resident) == (True, b.chunk)
    for resident in (cus, MAX_PER_CU * cus):
        assert plan_rows(rb, b.fixed, resident) == (False, 1)
    torch.cuda.empty_cache()
    free, need = torch.cuda.mem_get_info()[0], device_bytes(case, b)
    if free < need:
        pytest.skip(f"needs ~{need / 2 ** 30:.1f} GiB of free HBM, {free / 2 ** 30:.1f} GiB available")
    plan = make_plan(eng, case.shape)
    n = plan.n
    entry = getattr(plan, case.entry)

    def launch(operands, out, stream=None):
        entry(*operands, variant=case.variant, out=out, stream=stream)

    # the base block, and the entry point on it alone: one row per workgroup, all of them against the CPU reference
    host_a, host_b, want = blocks(case.shape, case.entry, P)
    base = [plan.to_device(h.astype(plan.dtype)) for h in (host_a, host_b) if h is not None]
    expected = torch.full((P, n), OUT_SENTINEL, dtype=plan.torch_dtype, device="cuda:0")
    launch(base, expected)
    differ = (plan.to_host(expected).astype(np.uint64) != want).any(axis=1).nonzero()[0]
    assert differ.size == 0, f"{P} rows, one per workgroup: {differ.size} differ from the CPU reference, the first {differ[:8].tolist()}"

    items = max(b.dynamic, b.captured)
    out = Guarded(plan.torch_dtype, items, n, b.chunk, OUT_SENTINEL)
    ins = [Guarded(plan.torch_dtype, items, n, b.chunk, IN_SENTINEL) for _ in base]
    problems = []                             # every launch is checked in full; the test fails at its end with all of them

    def arm(batch, shift):
        """Row r of every operand = row (r + shift) mod P of its base block; the output and everything around the rows of this
        launch hold the sentinels.  -> (the operands, the output, the expected block of this shift)"""
        out.reset()
        for g, blk in zip(ins, base):
            g.reset()
            fill_periodic(g.rows(batch), torch.roll(blk, -shift, 0))
        torch.cuda.synchronize()
        return [g.rows(batch) for g in ins], out.rows(batch), torch.roll(expected, -shift, 0)

    def check(batch, shift, exp, what):
        torch.cuda.synchronize()
        if not out.guards_intact(batch):
            problems.append((what, batch, "rows in front of or behind the output were written"))
        for k, (g, blk) in enumerate(zip(ins, base)):
            if not g.guards_intact(batch):
                problems.append((what, batch, f"rows in front of or behind operand {k} were written"))
            changed, first, _, _ = compare_periodic(g.rows(batch), torch.roll(blk, -shift, 0))
            if changed:
                problems.append((what, batch, f"rows of operand {k} changed", changed, "the first", first))
        differ, first_d, unwritten, first_u = compare_periodic(out.rows(batch), exp, OUT_SENTINEL)
        if unwritten:
            problems.append((what, batch, "rows never written", unwritten, "the first", first_u))
        if differ:
            problems.append((what, batch, "rows differ from the base block's", differ, "the first", first_d))

    # 1. rows from the device counter; the last chunk holds one row
    operands, view, exp = arm(b.dynamic, 0)
    launch(operands, view)
    check(b.dynamic, 0, exp, "dynamic")

    # 2. no counter pair: the same call captured into a graph (one kernel node, no parallel branches) and replayed twice, the
    #    inputs shifted by a row of the base block before each replay; the last chunk is one row short
    s1 = torch.cuda.Stream()
    operands, view, exp = arm(b.captured, 0)  # everything so far ran on the default stream: s1 starts behind it
    with torch.cuda.stream(s1):
        launch(operands, view, stream=s1)     # warm-up outside the capture: a live launch, rows from the counter
    s1.synchronize()
    check(b.captured, 0, exp, "warm-up")
    graph = torch.cuda.CUDAGraph()
    arm(b.captured, 0)
    with torch.cuda.graph(graph, stream=s1):
        launch(operands, view, stream=s1)
    for rep in range(2):
        _, _, exp = arm(b.captured, 1 + rep)
        with torch.cuda.stream(s1):
            graph.replay()
        s1.synchronize()
        check(b.captured, 1 + rep, exp, f"replay {rep}")
    del graph

    # 3. the fixed stride of single rows, every workgroup round its loop several times
    operands, view, exp = arm(b.fixed, 3)
    launch(operands, view)
    check(b.fixed, 3, exp, "fixed stride")
    assert not problems, "\n".join([f"{CASE_IDS[CASES.index(case)]}, chunk {b.chunk}, period {P}:"] + [" ".join(str(v) for v in p) for p in problems])
