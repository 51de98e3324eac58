"""The case table of tests/row_chunks.py against launch_plan.h's plan_rows, without a GPU: the condition that keeps
tests/test_gpu_row_chunks.py from passing vacuously.  Nothing on the device tells whether a launch took its rows from the counter,
so the batches must be dynamic, with a chunk of several rows and a ragged last chunk, for every number of resident workgroups
the occupancy query can return."""
import pytest

from row_chunks import CASES, CASE_IDS, MAX_PER_CU, batches, chosen_rows, plan_rows, row_bytes, shape_params

CUS = 256                       # compute units of an MI355X


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_both_batches_are_dynamic_with_a_ragged_last_chunk_and_a_slab_is_not(case):
    rb = row_bytes(case)
    b = batches(case, CUS)
    assert b.chunk >= 2
    assert b.chunk * rb >= 32768 > (b.chunk - 1) * rb               # the chunk is launch_plan.h's: 32 KiB per atomic, rounded up
    for batch in (b.dynamic, b.captured):
        assert batch >= b.threshold and batch % b.chunk != 0
        for per_cu in (1, 2, 4, 8, 16, 32):
            assert per_cu <= MAX_PER_CU
            assert plan_rows(rb, batch, per_cu * CUS) == (True, b.chunk), (batch, per_cu)
    assert b.dynamic % b.chunk == 1                                 # the last chunk holds one row
    assert b.captured % b.chunk == b.chunk - 1                      # the last chunk is one row short
    assert plan_rows(rb, b.slab, CUS) == (False, 1)                 # the fixed stride of single rows, the path the suite pins to the oracle
    assert plan_rows(rb, b.slab + 1, CUS) == (True, b.chunk)        # ... and the largest such batch
    for batch in (b.dynamic, b.captured):
        rows = chosen_rows(b.chunk, batch)
        assert rows[0] == 0 and rows[-1] == batch - 1 and all(0 <= r < batch for r in rows)
        assert {b.chunk - 1, b.chunk} <= set(rows) and batch - batch % b.chunk in rows


def test_every_family_has_a_case_in_each_lane_width():
    entries = {c.entry for c in CASES}
    assert len(entries) == 16
    for shape, word in (("S32", 4), ("S64", 8)):
        assert shape_params(shape)[3] == word
        assert {c.entry for c in CASES if c.shape == shape} == entries
    n, q, psi, _ = shape_params("S64")
    assert pow(psi, n, q) == q - 1                                  # a primitive 2n-th root
    assert len(set(CASE_IDS)) == len(CASES)


def test_chunks_of_the_table():
    """The chunk column of the table in the issue's words, computed: n * E rows 32 / 8, two terms 16 / 4, three terms 11 / 3,
    the external product and the CMux step 8 / 2, the blind rotation 4 / 2 (two steps / one)."""
    got = {}
    for case in CASES:
        got.setdefault((case.entry, case.terms), {})[case.shape] = batches(case, CUS).chunk
    assert got[("poly_mult", 1)] == got[("unprepare", 1)] == got[("ntt_inverse", 1)] == {"S32": 32, "S64": 8}
    assert got[("poly_dot_prepared", 2)] == got[("poly_galois_keyswitch_prepared", 2)] == {"S32": 16, "S64": 4}
    assert got[("poly_dot_prepared", 3)] == {"S32": 11, "S64": 3}
    assert got[("poly_external_product_prepared", 2)] == got[("poly_cmux_rotate_prepared", 2)] == {"S32": 8, "S64": 2}
    assert got[("poly_blind_rotate_prepared", 2)] == {"S32": 4, "S64": 2}
