"""The case table of the row-loop tests of the constant-geometry kernel (tests/test_gpu_cg_rows.py on the GPU,
tests/test_cg_rows_table.py without one): cg_kernel (csrc/cg_kernel_impl.h) at the smallest shapes at which each mechanism of its
row loop exists, the batches of the three launches of a case (launch_plan.h: plan_rows with the CG_ROWS policy) and the CPU
reference of a block of rows.  No torch here: the table, its arithmetic and the reference are checked without a GPU.

The mechanisms (cg_kernel_impl.h, "Row hand-out"):
  * single-trip shapes, log2 n == log2(2 GROUP): no barrier of a transform's own lies between the write of a next-row slot and
    its read, `if (ntrips == 1) __syncthreads()` is the only one;
  * GROUP 1 at n = 4: the largest chunk, 2,048 rows per atomic;
  * several trips with 64-bit lanes, where GROUP 8 has a product body of its own (AHEAD: both operands of the next row requested
    before the inverse transform);
  * the standalone-transform bodies and the cyclic product with a chunk above one row at a size that also has a fused kernel;
  * general plans, which stage the twiddle table twice inside every product row (CG_FLAG_RESTAGE);
  * an omega-only plan."""
import ctypes
from collections import namedtuple

import numpy as np

import emu_library
from conftest import PARAMS
from emu_library import smallest_dynamic_batch
from row_chunks import MAX_PER_CU, Q60

CG = 1                          # emu_plan_rows / emu_row_policy: the constant-geometry kernels' policy
Q23 = 8380417
ENTRIES = ("poly_mult", "cyclic_poly_mult", "ntt_forward", "ntt_inverse", "twisted_ntt_forward")
PRODUCTS = ("poly_mult", "cyclic_poly_mult")

# kind: "plan" (validated: root is psi), "general" (tn_plan_create_general: root is psi, nothing validated), "omega"
# (tn_plan_create_omega: root is omega).  root None: the smallest primitive 2n-th root.  word: bytes per lane.
Shape = namedtuple("Shape", "kind n q root word")
SHAPES = {
    "T16": Shape("plan", 16, Q23, None, 4),                 # single trip at GROUP 8
    "T8": Shape("plan", 8, Q23, None, 4),                   # ... at GROUP 4
    "T4": Shape("plan", 4, Q23, None, 4),                   # ... at GROUP 2; at GROUP 1 two trips and the largest chunk
    "M64": Shape("plan", 64, Q60, None, 8),                 # several trips, 64-bit lanes
    "F1024": Shape("plan", *PARAMS["P1024"], 4),            # a fused size: the chunk of 8 rows
    "G64": Shape("general", 64, 1000000, 3, 4),             # an even modulus, 32-bit lanes (tests/test_gpu_galois.py)
    "G16": Shape("general", 16, 2305843009213693950, 12345678901234567, 8),      # an even modulus of 61 bits (tests/golden: general_psi)
    "W32": Shape("omega", 32, 7681, 3, 4),                  # omega-only (tests/test_gpu_galois.py)
}


def shape_params(name):
    """-> (kind, n, q, psi or None, omega, bytes per word)"""
    s = SHAPES[name]
    if s.kind == "omega":
        return s.kind, s.n, s.q, None, s.root, s.word
    psi = s.root
    if psi is None:
        from tiny_ntt_amd import numtheory
        psi = numtheory.primitive_2n_root(s.n, s.q)
    return s.kind, s.n, s.q, psi, psi * psi % s.q, s.word


Case = namedtuple("Case", "shape entry variant")


def _cases():
    out = []

    def add(shape, entries, variants):
        out.extend(Case(shape, e, v) for v in variants for e in entries)
    add("T16", ENTRIES, ("cg8",))
    add("T16", ("poly_mult",), ("cg8_padded",))             # (the layouts differ at n = 4096 / 60-bit alone: the dispatcher's other arm)
    add("T8", ("poly_mult",), ("cg4",))
    add("T4", ("poly_mult",), ("cg2",))
    add("T4", ("poly_mult", "ntt_forward"), ("cg",))
    add("M64", ENTRIES, ("cg8",))
    add("M64", ("poly_mult", "ntt_inverse"), ("cg4_padded",))
    add("F1024", ENTRIES[1:], ("cg", "cg8_padded"))         # (the negacyclic product at this shape: tests/test_gpu_parity.py)
    for shape in ("G64", "G16"):
        add(shape, ("poly_mult", "ntt_forward", "ntt_inverse"), ("cg", "cg8"))
    add("W32", ("ntt_forward", "ntt_inverse"), ("cg8",))
    return out


CASES = _cases()
CASE_IDS = [f"{c.shape}-{c.entry}-{c.variant}" for c in CASES]


def group_of(case):
    """Butterflies per lane-step the dispatcher runs the variant with (kernels.hip: launch_cg halves the group until a lane-step
    holds no more than the polynomial)."""
    digits = "".join(ch for ch in case.variant.split("_")[0] if ch.isdigit())
    group, n = int(digits or 1), SHAPES[case.shape].n
    while 2 * group > n:
        group //= 2
    return group


def single_trip(case):
    return SHAPES[case.shape].n == 2 * group_of(case)


def row_bytes(case):
    s = SHAPES[case.shape]
    return s.n * s.word


def plan_rows(row_bytes_, batch, resident):
    """launch_plan.h's plan_rows with the CG_ROWS policy -> (rows come from the device counter, rows per hand-out)."""
    L = emu_library.load()
    sz = ctypes.c_size_t
    L.emu_plan_rows.argtypes = [ctypes.c_int, sz, sz, sz, ctypes.POINTER(ctypes.c_uint32)]
    chunk = ctypes.c_uint32()
    dynamic = L.emu_plan_rows(CG, row_bytes_, batch, resident, ctypes.byref(chunk))
    return bool(dynamic), chunk.value


Batches = namedtuple("Batches", "chunk threshold dynamic captured fixed")


def batches(case, cus):
    """The batches of a case's three launches on a device of `cus` compute units.
    threshold: the smallest batch that plan_rows hands out through the counter when MAX_PER_CU workgroups per CU are resident;
    plan_rows is monotone in `resident`, so a batch at or above it is dynamic with the same chunk whatever the occupancy query
    returns.  dynamic: the last chunk holds one row.  captured: the last chunk is one row short.
    fixed: below the threshold with ONE workgroup per CU resident, 8 * cus * chunk, so the launch keeps the fixed stride of
    single rows for any occupancy; 4 * MAX_PER_CU * cus + 1 rows where that is below it, so that every workgroup takes four
    rows and more whatever the occupancy.  With a chunk of 16 rows and fewer (here: 8, at n = 1024 / 32-bit) no batch is both,
    and the launch is the largest that keeps the fixed stride, 64 * cus - 1 rows: three rows and more per workgroup while at
    most 16 workgroups are resident per CU, two (and one workgroup with one) at 32."""
    rb = row_bytes(case)
    threshold = smallest_dynamic_batch(rb, MAX_PER_CU * cus, CG)
    _, chunk = plan_rows(rb, threshold, MAX_PER_CU * cus)
    fixed = min(4 * MAX_PER_CU * cus + 1, smallest_dynamic_batch(rb, cus, CG) - 1)
    return Batches(chunk, threshold, threshold + chunk + 1, threshold + 2 * chunk - 1, fixed)


def period(cus):
    """P, the number of base rows: the largest prime that is at most `cus`, does not divide it and is above 128.  A prime above
    MAX_PER_CU that does not divide the CU count is coprime to every chunk (a power of two), to every grid (workgroups per CU,
    at most MAX_PER_CU, times the CU count) and to their products, so no hand-out error, which displaces rows by multiples of
    the chunk or of grid * chunk, maps a row onto another with the same expected words; and P rows at most `cus` are one row
    per workgroup for any occupancy."""
    for p in range(cus, 128, -1):
        if cus % p and all(p % d for d in range(2, int(p ** 0.5) + 1)):
            return p
    raise ValueError(f"no prime above 128 among 129 ... {cus}")


def device_bytes(case, b):
    """What a case allocates at most, for the skip when the device has less free: every operand and the output at the largest
    batch with their guard rows, and room for the comparisons' temporaries."""
    operands = 2 if case.entry in PRODUCTS else 1
    return (operands + 1) * (max(b.dynamic, b.captured) + 2 * b.chunk) * row_bytes(case) + (1 << 29)


def base_rows(case_shape, rows, operand):
    """The base block of an operand: `rows` rows of words below q, row 0 all q - 1; the same for every case of a shape."""
    s = SHAPES[case_shape]
    rng = np.random.default_rng([s.n, s.word, operand])
    x = rng.integers(0, s.q, (rows, s.n), dtype=np.uint64)
    x[0] = s.q - 1
    return x


def mulmod_rows(x, y, q):
    """x * y mod q, element by element, in Python integers (q may have 61 bits)."""
    return np.array((x.astype(object) * y.astype(object)) % q, dtype=np.uint64)


def reference(oracle, shape, entry, a, b=None):
    """The entry point on the rows of a (and b) from the CPU reference: oracle.poly_mult (cg_ntt.py:78-92, whatever psi and the
    modulus are), python_poly_mult for the cyclic product (tests/test_gpu_next.py: cyclic_oracle), cg_ntt / cg_intt with the
    plan's omega, and the twist by psi^i in front of cg_ntt (benchmark_ntt_60bit.cpp:161-165, forward_ntt_bench)."""
    _, n, q, psi, omega, _ = shape_params(shape)
    if entry == "poly_mult":
        return oracle.poly_mult(a, b, q, psi)
    if entry == "cyclic_poly_mult":
        A = np.stack([oracle.cg_ntt(x, omega, q) for x in a])
        B = np.stack([oracle.cg_ntt(x, omega, q) for x in b])
        return np.stack([oracle.cg_intt(x, omega, q) for x in mulmod_rows(A, B, q)])
    if entry == "ntt_forward":
        return np.stack([oracle.cg_ntt(x, omega, q) for x in a])
    if entry == "ntt_inverse":
        return np.stack([oracle.cg_intt(x, omega, q) for x in a])
    assert entry == "twisted_ntt_forward"
    twist = np.array([pow(psi, i, q) for i in range(n)], dtype=np.uint64)
    return np.stack([oracle.cg_ntt(x, omega, q) for x in mulmod_rows(a, twist[None, :], q)])
