"""The case table of tests/cg_rows.py against launch_plan.h's plan_rows with the constant-geometry policy, without a GPU: the
condition that keeps tests/test_gpu_cg_rows.py from passing vacuously.  Nothing on the device tells whether a launch took its rows
from the counter or how many rows a workgroup ran, so the batches must be dynamic, with a chunk of several rows and a ragged last
chunk, for every number of resident workgroups the occupancy query can return, and the fixed-stride batch must stay fixed."""
import numpy as np
import pytest

from cg_rows import (CASES, CASE_IDS, ENTRIES, MAX_PER_CU, SHAPES, batches, base_rows, group_of, period, plan_rows, reference,
                     row_bytes, shape_params, single_trip)

CUS = 256                       # compute units of an MI355X
PER_CU = (1, 2, 4, 8, 16, 32)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_the_three_batches_of_a_case(case):
    rb = row_bytes(case)
    b = batches(case, CUS)
    assert b.chunk >= 2
    assert b.chunk * rb >= 32768 > (b.chunk - 1) * rb               # the chunk is launch_plan.h's: 32 KiB per atomic, rounded up
    for batch in (b.dynamic, b.captured):
        assert batch >= b.threshold and batch % b.chunk != 0
        for per_cu in PER_CU:
            assert per_cu <= MAX_PER_CU
            assert plan_rows(rb, batch, per_cu * CUS) == (True, b.chunk), (batch, per_cu)
    assert b.dynamic % b.chunk == 1                                 # the last chunk holds one row
    assert b.captured % b.chunk == b.chunk - 1                      # the last chunk is one row short
    # the fixed stride of single rows whatever the occupancy, and every workgroup goes round its loop
    for per_cu in PER_CU:
        assert plan_rows(rb, b.fixed, per_cu * CUS) == (False, 1), per_cu
    if b.chunk > 16:
        assert b.fixed == 4 * MAX_PER_CU * CUS + 1
    else:                       # no batch is both below 8 * CUS * chunk and above 4 * MAX_PER_CU * CUS: the largest fixed one
        assert 8 * CUS * b.chunk <= 4 * MAX_PER_CU * CUS
        assert plan_rows(rb, b.fixed + 1, CUS) == (True, b.chunk)
        assert b.fixed >= 3 * 16 * CUS and b.fixed > MAX_PER_CU * CUS


def test_chunks_of_the_table():
    got = {shape: {batches(c, CUS).chunk for c in CASES if c.shape == shape} for shape in SHAPES}
    assert got == {"T16": {512}, "T8": {1024}, "T4": {2048}, "M64": {64}, "F1024": {8}, "G64": {128}, "G16": {256}, "W32": {256}}
    # 8 * 32 * 256 chunks of 32 KiB: 2 GiB per operand whatever n is
    for case in CASES:
        b = batches(case, CUS)
        assert b.threshold * row_bytes(case) == 2 ** 31
        assert max(b.dynamic, b.captured) * row_bytes(case) < 2 ** 31 + 2 ** 17


def test_every_mechanism_of_the_issue_has_its_cases():
    have = {(c.shape, c.variant): set() for c in CASES}
    for c in CASES:
        have[(c.shape, c.variant)].add(c.entry)
    assert len(set(CASE_IDS)) == len(CASES) == 39
    # single-trip shapes, 32-bit lanes
    assert have[("T16", "cg8")] == set(ENTRIES) and "poly_mult" in have[("T16", "cg8_padded")]
    assert "poly_mult" in have[("T8", "cg4")] and "poly_mult" in have[("T4", "cg2")]
    for c in CASES:
        # (the general plan at n = 16 is a single trip at GROUP 8 too: its extra barrier and the re-staging in one row)
        assert single_trip(c) == ((c.shape, group_of(c)) in (("T16", 8), ("T8", 4), ("T4", 2), ("G16", 8))), c
        assert 2 * group_of(c) <= SHAPES[c.shape].n
    assert all(SHAPES[s].word == 4 and SHAPES[s].q == 8380417 for s in ("T16", "T8", "T4"))
    # GROUP 1 at n = 4, several trips with 64-bit lanes, the transform bodies at a fused size
    assert have[("T4", "cg")] == {"poly_mult", "ntt_forward"}
    assert have[("M64", "cg8")] == set(ENTRIES) and have[("M64", "cg4_padded")] == {"poly_mult", "ntt_inverse"}
    assert SHAPES["M64"].word == 8 and SHAPES["M64"].q == 2 ** 60 - 2 ** 14 + 1
    for v in ("cg", "cg8_padded"):
        assert have[("F1024", v)] == set(ENTRIES) - {"poly_mult"}
    # general plans in both lane widths, an omega-only plan
    for s, word in (("G64", 4), ("G16", 8)):
        assert SHAPES[s].kind == "general" and SHAPES[s].word == word and SHAPES[s].q % 2 == 0
        for v in ("cg", "cg8"):
            assert have[(s, v)] == {"poly_mult", "ntt_forward", "ntt_inverse"}
    assert SHAPES["W32"].kind == "omega" and have[("W32", "cg8")] == {"ntt_forward", "ntt_inverse"}
    for s in ("T16", "T8", "T4", "M64", "F1024"):
        _, n, q, psi, omega, _ = shape_params(s)
        assert pow(psi, n, q) == q - 1 and omega == psi * psi % q       # a primitive 2n-th root


def test_the_period_is_coprime_to_every_chunk_and_grid():
    p = period(CUS)
    assert p == 251 and 128 < p <= CUS
    for case in CASES:
        chunk = batches(case, CUS).chunk
        for per_cu in range(1, MAX_PER_CU + 1):
            assert chunk % p and (per_cu * CUS) % p and (per_cu * CUS * chunk) % p
    assert period(304) == 293 and period(257) == 251                 # a prime CU count is not its own period
    with pytest.raises(ValueError):
        period(128)


def test_the_p256_launches_of_the_existing_test_are_dynamic_with_one_workgroup_per_cu_alone():
    """tests/test_gpu_parity.py::test_constant_geometry_kernels_take_rows_from_the_counter_like_the_fused_ones launches 70,000,
    40,001 and 515 rows at n = 256 / 32-bit lanes (rows of 1 KiB, a chunk of 32).  plan_rows calls a launch dynamic from
    8 * resident * 32 rows: 65,536 with one workgroup per CU resident, 131,072 with two.  So the largest of them takes its rows
    from the counter only if the occupancy query returns one workgroup per CU, and these kernels (64 to 128 threads at n = 256)
    fit several: at P256 that test runs the fixed stride of single rows.  Its launches at n = 2048 / 60-bit (20,001 rows, chunk
    2) and n = 1024 / 24-bit (200,003 rows, chunk 8) are dynamic up to 4 and 12 workgroups per CU, in product mode alone.  The
    fact is kept here so that the gap tests/test_gpu_cg_rows.py closes stays documented; that test is unchanged."""
    assert plan_rows(1024, 70000, CUS) == (True, 32)
    for per_cu in PER_CU[1:]:
        assert plan_rows(1024, 70000, per_cu * CUS) == (False, 1), per_cu
    for rows in (40001, 515):
        for per_cu in PER_CU:
            assert plan_rows(1024, rows, per_cu * CUS) == (False, 1), (rows, per_cu)
    assert [plan_rows(16384, 20001, per_cu * CUS)[0] for per_cu in PER_CU] == [True, True, True, False, False, False]
    assert [plan_rows(4096, 200003, per_cu * CUS)[0] for per_cu in PER_CU] == [True, True, True, True, False, False]


def test_the_cpu_reference_of_a_block(oracle, golden):
    """cg_rows.reference on known answers: the twisted forward transform on the golden vector of the reference benchmark, the
    transforms as inverses of each other, the cyclic product's wrap-around, and the negacyclic product against the O(n^2) one."""
    g = golden("P1024")
    assert np.array_equal(reference(oracle, "F1024", "twisted_ntt_forward", g["lcg12_mul_a"][None, :])[0], g["lcg1_fwd"])
    for shape in ("T16", "M64"):
        _, n, q, psi, omega, _ = shape_params(shape)
        a, b = base_rows(shape, 3, 0), base_rows(shape, 3, 1)
        assert a.shape == (3, n) and int(a.max()) < q and (a[0] == q - 1).all() and not np.array_equal(a, b)
        assert np.array_equal(reference(oracle, shape, "ntt_inverse", reference(oracle, shape, "ntt_forward", a)), a)
        xm = np.zeros((1, n), dtype=np.uint64); xm[0, n - 1] = 1
        x1 = np.zeros((1, n), dtype=np.uint64); x1[0, 1] = 1
        assert reference(oracle, shape, "cyclic_poly_mult", xm, x1)[0, 0] == 1
        assert reference(oracle, shape, "poly_mult", xm, x1)[0, 0] == q - 1
        c = reference(oracle, shape, "poly_mult", a, b)
        assert all(np.array_equal(c[r], oracle.schoolbook(a[r], b[r], q)) for r in range(3))
