"""The case table of the row hand-out tests (tests/test_gpu_row_chunks.py on the GPU, tests/test_row_chunks_table.py without one):
every persistent fused kernel at the two smallest shapes whose rows are handed out in chunks of several rows, with the row size
its launcher plans with (the launch_persistent calls of csrc/kernels*.hip) and the batches that make a launch dynamic whatever
the occupancy query returns.  No torch here: the table and its arithmetic are checked without a GPU."""
import ctypes
from collections import namedtuple

import emu_library
from conftest import PARAMS
from emu_library import smallest_dynamic_batch

Q60 = 1152921504606830593
MAX_PER_CU = 32          # a CU holds at most 32 waves and a workgroup has at least one: the occupancy query returns no more


def shape_params(shape):
    """S32: n = 256 / 23-bit q, 32-bit lanes, rows of 1 KiB.  S64: n = 512 / 60-bit q, 64-bit lanes, rows of 4 KiB.
    -> (n, q, psi, bytes per word)"""
    if shape == "S32":
        return PARAMS["P256"] + (4,)
    from tiny_ntt_amd import numtheory
    assert shape == "S64"
    return 512, Q60, numtheory.primitive_2n_root(512, Q60), 8


# entry: the Python name of the entry point.  mult: the launcher plans a row of mult * n * E bytes.  in_rows, key_rows, out_rows:
# rows of n words per batch item of the input, of a key per item (shared: one key for all) and of the output.  mode: what else
# tells two cases of one entry point apart.
Case = namedtuple("Case", "entry shape mult terms steps shared mode in_rows key_rows out_rows")


def _cases():
    out = []
    for shape in ("S32", "S64"):
        def add(entry, mult=1, terms=1, steps=1, shared=None, mode=None, in_rows=1, key_rows=0, out_rows=1):
            out.append(Case(entry, shape, mult, terms, steps, shared, mode, in_rows, key_rows, out_rows))
        for entry in ("poly_mult", "cyclic_poly_mult"):
            add(entry, in_rows=2)
        for entry in ("ntt_forward", "ntt_inverse", "twisted_ntt_forward", "prepare", "unprepare"):
            add(entry)
        for shared in (True, False):
            add("poly_mult_prepared", shared=shared, key_rows=1)
            for terms in (2, 3):      # a row of 3 operand rows does not divide 32 KiB: plan_rows rounds the chunk up
                add("poly_dot_prepared", terms, terms, shared=shared, in_rows=terms, key_rows=terms)
            for mode in ("coefficients", "keep_prepared"):
                add("poly_dot_hat", 2, 2, shared=shared, mode=mode, in_rows=2, key_rows=2)
            add("poly_gadget_dot_prepared", 2, 2, shared=shared, key_rows=2)
            add("poly_gadget_multidot_prepared", 2, 2, shared=shared, key_rows=4, out_rows=2)
            add("poly_galois_keyswitch_prepared", 2, 2, shared=shared, in_rows=2, key_rows=4, out_rows=2)
            add("poly_external_product_prepared", 4, 2, shared=shared, in_rows=2, key_rows=8, out_rows=2)
            add("poly_cmux_rotate_prepared", 4, 2, shared=shared, in_rows=2, key_rows=8, out_rows=2)
        # 2 * terms * steps operand rows: with two steps a row of the 64-bit shape is 32 KiB, a chunk of one
        steps = 2 if shape == "S32" else 1
        for mode in ("separate", "in_place"):
            add("poly_blind_rotate_prepared", 4 * steps, 2, steps, shared=True, mode=mode, in_rows=2, out_rows=2)
    return out


CASES = _cases()


def case_id(case):
    parts = [case.entry, case.shape]
    if case.terms > 1:
        parts.append(f"terms{case.terms}")
    if case.steps > 1 or case.entry == "poly_blind_rotate_prepared":
        parts.append(f"steps{case.steps}")
    if case.shared is not None and case.entry != "poly_blind_rotate_prepared":
        parts.append("shared" if case.shared else "per_row")
    if case.mode:
        parts.append(case.mode)
    return "-".join(parts)


CASE_IDS = [case_id(c) for c in CASES]


def row_bytes(case):
    n, _, _, word = shape_params(case.shape)
    return case.mult * n * word


def plan_rows(row_bytes_, batch, resident):
    """launch_plan.h's plan_rows for the fused kernels -> (rows come from the device counter, rows per hand-out)."""
    L = emu_library.load()
    sz = ctypes.c_size_t
    L.emu_plan_rows.argtypes = [ctypes.c_int, sz, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    chunk = ctypes.c_uint32()
    dynamic = L.emu_plan_rows(0, row_bytes_, batch, resident, ctypes.byref(chunk))
    return bool(dynamic), chunk.value


Batches = namedtuple("Batches", "chunk threshold dynamic captured slab")


def batches(case, cus):
    """The batches of a case on a device of `cus` compute units.  threshold: the smallest batch that plan_rows hands out through
    the counter when MAX_PER_CU workgroups per CU are resident; plan_rows is monotone in `resident`, so a batch at or above it
    is dynamic with the same chunk for whatever the occupancy query returns.  dynamic: the last chunk holds one row.  captured:
    the last chunk is one row short.  slab: below 4 * cus * chunk, the threshold with ONE workgroup per CU resident, so a launch
    of a slab runs the fixed stride of single rows for any occupancy."""
    rb = row_bytes(case)
    threshold = smallest_dynamic_batch(rb, MAX_PER_CU * cus)
    _, chunk = plan_rows(rb, threshold, MAX_PER_CU * cus)
    return Batches(chunk, threshold, threshold + chunk + 1, threshold + 2 * chunk - 1, 4 * cus * chunk - 1)


def chosen_rows(chunk, batch):
    """The rows compared with the CPU reference: the first two, both sides of the first chunk boundary, both sides of a boundary
    in the middle of the launch, and every row of the ragged last chunk."""
    mid = batch // 2 // chunk * chunk
    last = (batch - 1) // chunk * chunk
    return sorted({0, 1, chunk - 1, chunk, chunk + 1, mid - 1, mid} | set(range(last, batch)))


def device_bytes(case, b):
    """What a case allocates at most, for the skip when the device has less free: the input, a key per item, the output and the
    expected rows of the larger batch with their guard rows, once more the input and the key where they are prepared from raw
    rows, and a quarter on top for the comparisons' temporaries."""
    n, _, _, word = shape_params(case.shape)
    rows = 2 * case.in_rows + 2 * (0 if case.shared else case.key_rows) + 3 * case.out_rows
    return (max(b.dynamic, b.captured) + b.chunk) * rows * n * word * 5 // 4 + (1 << 28)
