"""One table of calls of the device entry points and what each must answer: status and tn_last_error text.

The same rows go to the CPU stepping of the argument checks (emu_api_check, tests/test_api_checks_emu.py) and to the real
library (tests/test_gpu_api_cases.py).  The statuses are those the test_status_codes blocks of tests/test_gpu_{prepared,dot,
hat,gadget}.py and test_gpu_next.py::test_overlapping_output_is_rejected_and_many_streams_stay_correct assert; the texts are
what the library answered before the checks moved into csrc/api_checks.h.

A row names its plan by kind (FUSED: tn_plan_create with the fused kernels; GENERAL: tn_plan_create_general, no fused kernels;
OMEGA: tn_plan_create_omega; NULL) and its pointers by place: None, DUMMY (address 4096: only in rows that are refused before
anything is read), or (buffer, rows) - `rows` rows past the start of buffer "A", "B" or "OUT".  The buffers lie in one arena,
ARENA_ROWS rows long, with MARGIN rows before the first and between any two, so that every pointer of a row is owned memory."""
import ctypes
from collections import namedtuple

OK, EINVAL, EUNSUPPORTED = 0, 6, 7
FUSED, GENERAL, OMEGA, NULL = "fused", "general", "omega", "null"
DUMMY = "dummy"
MARGIN, SPAN = 16, 16                       # rows: margin before each buffer, rows of a buffer (>= batch * terms + terms)
FIRST_ROW = {"A": MARGIN, "B": 2 * MARGIN + SPAN, "OUT": 3 * MARGIN + 2 * SPAN}
ARENA_ROWS = 3 * (MARGIN + SPAN)

Case = namedtuple("Case", "id entry plan args status text launches")

T_PLAN = "{fn}: plan is NULL"
T_BUFFER = "{fn}: NULL buffer"
T_ARGUMENT = "{fn}: NULL argument"
T_FUSED = "{fn}: prepared operands need a plan with the fused kernels (tn_plan_has_fused)"
T_TERMS = "{fn}: terms must be at least 1"
T_ROWS = "{fn}: batch too large for one call (max 2^31 - 1 rows)"
T_ROWS2 = "{fn}: batch * terms too large for one call (max 2^31 - 1 {noun})"
T_WIDE = "{fn}: batch too large"
T_BHAT_ROWS = "{fn}: bhat_rows must be 1 (shared operand) or batch"
T_SETS = "{fn}: bhat_sets must be 1 (one set of operands for every row) or batch"
T_KEEP = "{fn}: out_prepared must be 0 (coefficients) or 1 (prepared rows)"
T_FLAG = "{fn}: unknown flag bit"
T_BASE = "{fn}: need 1 <= base_log and 2^base_log < q"
T_SHIFT = "{fn}: (terms - 1) * base_log must be below 64"
T_OVERLAP = "{fn}: output must not alias or overlap an input"
T_OVERLAP_THE = "{fn}: output must not alias or overlap the input"
T_OMEGA = {"tn_poly_mult_dev": "{fn}: an omega-only plan has no psi (tn_plan_create_omega offers cg_ntt / cg_intt only)",
           "tn_cyclic_poly_mult_dev": "{fn}: not available on an omega-only plan",
           "tn_twisted_ntt_forward_dev": "{fn}: an omega-only plan has no psi to twist with"}
NOUN = {"tn_poly_dot_prepared_dev": "rows of a", "tn_poly_dot_hat_dev": "rows of ahat", "tn_poly_gadget_dot_prepared_dev": "digit rows",
        "tn_gadget_decompose_dev": "digit rows"}


def cases(batch, terms, k):
    """The table for a plan whose modulus has k bits, the sizes of an ordinary call being (batch, terms)."""
    assert batch >= 4 and terms >= 2 and batch * terms + terms <= SPAN and batch * terms - 1 <= MARGIN
    w = 30 if k > 31 else 12                                   # a base_log with 2^w < q and (terms - 1) * w < 64
    rows = []

    def add(id_, entry, status=OK, text=None, plan=FUSED, launches=None, **args):
        full = dict(a=("A", 0), b=("B", 0), out=("OUT", 0), sets=batch, batch=batch, terms=terms, out_prepared=0, base_log=w, flags=0)
        full.update(args)
        assert (status == OK) == (text is None)
        text = text.format(fn=entry, noun=NOUN.get(entry)) if text else None
        rows.append(Case(f"{entry[3:-4]}-{id_}", entry, plan, full, status, text, status == OK if launches is None else launches))

    # ---- a, b -> c row by row: the products, the direct product, the pointwise product ----
    for e in ("tn_poly_mult_dev", "tn_cyclic_poly_mult_dev", "tn_schoolbook_dev"):
        add("ok", e)
        if e != "tn_schoolbook_dev":
            add("general-plan", e, plan=GENERAL)
        add("null-plan", e, EINVAL, T_PLAN, plan=NULL)
        for name in ("a", "b", "out"):
            add(f"null-{name}", e, EINVAL, T_BUFFER, **{name: None})
        add("batch0-null", e, a=None, b=None, out=None, batch=0)               # these go on to a launch of no rows
        add("rows-2^31", e, EINVAL, T_ROWS, batch=2 ** 31)
        add("out-is-a", e, EINVAL, T_OVERLAP, out=("A", 0))
        add("out-is-b", e, EINVAL, T_OVERLAP, out=("B", 0))
        # test_gpu_next: a = buf[0:4], b = buf[4:8], c = buf[2:6] overlaps the tail of a and the head of b
        add("out-over-tail-of-a-and-head-of-b", e, EINVAL, T_OVERLAP, b=("A", 4), out=("A", 2), batch=4)
        add("out-first-row-is-last-of-b", e, EINVAL, T_OVERLAP, out=("B", batch - 1))
        add("out-last-row-is-first-of-b", e, EINVAL, T_OVERLAP, out=("B", 1 - batch))
        add("out-just-past-a", e, out=("A", batch))
    for e in ("tn_poly_mult_dev", "tn_cyclic_poly_mult_dev"):
        add("omega-plan", e, EUNSUPPORTED, T_OMEGA[e], plan=OMEGA)
        add("omega-plan-null-a", e, EINVAL, T_BUFFER, plan=OMEGA, a=None)       # the buffers are looked at first
    e = "tn_pointwise_mul_dev"
    add("ok", e)
    add("in-place", e, out=("A", 0))
    add("omega-plan", e, plan=OMEGA)
    add("null-plan", e, EINVAL, T_PLAN, plan=NULL)
    for name in ("a", "b", "out"):
        add(f"null-{name}", e, EINVAL, T_BUFFER, **{name: None})
    add("batch0-null", e, a=None, b=None, out=None, batch=0)
    add("rows-2^32", e, EINVAL, T_WIDE, batch=2 ** 32)
    add("rows-2^32-null-a", e, EINVAL, T_WIDE, batch=2 ** 32, a=None)            # the size is looked at first

    # ---- in -> out row by row: the transforms, prepare and unprepare ----
    for e in ("tn_ntt_forward_dev", "tn_ntt_inverse_dev", "tn_twisted_ntt_forward_dev", "tn_prepare_dev", "tn_unprepare_dev"):
        n_rows = batch * terms if e == "tn_unprepare_dev" else batch
        add("ok", e, batch=n_rows)
        add("null-plan", e, EINVAL, T_PLAN, plan=NULL)
        add("null-in", e, EINVAL, T_BUFFER, a=None)
        add("null-out", e, EINVAL, T_BUFFER, out=None)
        add("rows0-null", e, a=None, out=None, batch=0)
        add("rows-2^31-dummy" if e == "tn_unprepare_dev" else "rows-2^31", e, EINVAL, T_ROWS, batch=2 ** 31,
            **(dict(a=DUMMY, out=DUMMY) if e == "tn_unprepare_dev" else {}))
        add("out-is-in", e, EINVAL, T_OVERLAP, out=("A", 0), batch=n_rows)
        add("out-first-row-is-last-of-in", e, EINVAL, T_OVERLAP, out=("A", n_rows - 1), batch=n_rows)
        add("out-last-row-is-first-of-in", e, EINVAL, T_OVERLAP, out=("A", 1 - n_rows), batch=n_rows)
        add("out-just-past-in", e, out=("A", batch))
    add("out-over-tail-of-in", "tn_ntt_forward_dev", EINVAL, T_OVERLAP, out=("A", 3), batch=4)     # test_gpu_next: buf[0:4] -> buf[3:7]
    for e in ("tn_ntt_forward_dev", "tn_ntt_inverse_dev"):
        add("omega-plan", e, plan=OMEGA)
    add("omega-plan", "tn_twisted_ntt_forward_dev", EUNSUPPORTED, T_OMEGA["tn_twisted_ntt_forward_dev"], plan=OMEGA)
    for e in ("tn_prepare_dev", "tn_unprepare_dev"):
        for plan in (GENERAL, OMEGA):
            add(f"{plan}-plan", e, EUNSUPPORTED, T_FUSED, plan=plan)
        add("general-plan-null-out", e, EINVAL, T_BUFFER, plan=GENERAL, out=None)   # buffers and overlap come before the plan's kernels
        add("general-plan-out-is-in", e, EINVAL, T_OVERLAP, plan=GENERAL, out=("A", 0))

    # ---- tn_poly_mult_prepared_dev ----
    e = "tn_poly_mult_prepared_dev"
    add("ok", e)
    add("shared-ok", e, sets=1)
    add("null-plan", e, EINVAL, T_PLAN, plan=NULL)
    for plan in (GENERAL, OMEGA):
        add(f"{plan}-plan", e, EUNSUPPORTED, T_FUSED, plan=plan)
    add("general-plan-null-a", e, EUNSUPPORTED, T_FUSED, plan=GENERAL, a=None)      # the plan's kernels come first here
    add("rows-2^31", e, EINVAL, T_ROWS, batch=2 ** 31)
    for name in ("a", "b", "out"):
        add(f"null-{name}", e, EINVAL, T_BUFFER, **{name: None})
    add("batch0-null", e, a=None, b=None, out=None, sets=1, batch=0, launches=False)
    add("batch0-sets2", e, sets=2, batch=0, launches=False)
    add("sets-2", e, EINVAL, T_BHAT_ROWS, sets=2)
    add("null-a-sets-2", e, EINVAL, T_BUFFER, sets=2, a=None)
    add("out-is-a", e, EINVAL, T_OVERLAP, out=("A", 0))
    add("out-is-bhat", e, EINVAL, T_OVERLAP, out=("B", 0))
    add("out-last-row-is-the-shared-row", e, EINVAL, T_OVERLAP, sets=1, out=("B", 1 - batch))
    add("out-over-tail-of-a", e, EINVAL, T_OVERLAP, out=("A", 2), batch=3, sets=3)
    add("out-just-past-the-shared-row", e, sets=1, out=("B", 1))

    # ---- the three dot products ----
    for e, keep in (("tn_poly_dot_prepared_dev", 0), ("tn_poly_dot_hat_dev", 0), ("tn_poly_dot_hat_dev", 1), ("tn_poly_gadget_dot_prepared_dev", 0)):
        gadget = e == "tn_poly_gadget_dot_prepared_dev"
        a_rows = batch if gadget else batch * terms
        kw = dict(out_prepared=keep)
        tag = "keep-" if keep else ""
        add(tag + "ok", e, **kw)
        add(tag + "shared-ok", e, sets=1, **kw)
        add(tag + "out-is-a", e, EINVAL, T_OVERLAP, out=("A", 0), **kw)
        add(tag + "out-is-bhat", e, EINVAL, T_OVERLAP, out=("B", 0), **kw)
        add(tag + "out-first-row-is-last-of-a", e, EINVAL, T_OVERLAP, out=("A", a_rows - 1), **kw)
        add(tag + "out-first-row-is-last-of-shared-set", e, EINVAL, T_OVERLAP, sets=1, out=("B", terms - 1), **kw)
        add(tag + "out-last-row-is-first-of-a", e, EINVAL, T_OVERLAP, out=("A", 1 - batch), **kw)
        add(tag + "out-last-row-is-first-of-shared-set", e, EINVAL, T_OVERLAP, sets=1, out=("B", 1 - batch), **kw)
        add(tag + "out-just-past-the-shared-set", e, sets=1, out=("B", terms), batch=1, **kw)
        add(tag + "out-just-past-a", e, out=("A", a_rows), **kw)
        for plan in (GENERAL, OMEGA):
            add(tag + f"{plan}-plan", e, EUNSUPPORTED, T_FUSED, plan=plan, sets=1 if gadget else 2, batch=2, terms=2, **kw)
        if keep:
            continue
        add("null-plan", e, EINVAL, T_PLAN, plan=NULL)
        for name in ("a", "b", "out"):
            add(f"null-{name}", e, EINVAL, T_BUFFER, **{name: None})
        add("terms-0", e, EINVAL, T_TERMS, terms=0)
        add("terms-0-general-plan", e, EUNSUPPORTED, T_FUSED, plan=GENERAL, terms=0)
        add("sets-2", e, EINVAL, T_SETS, sets=2)
        add("sets-2-null-a", e, EINVAL, T_BUFFER, sets=2, a=None)
        add("batch0-null", e, a=None, b=None, out=None, sets=1, batch=0, terms=3, base_log=min(20, w), launches=False)
        if not gadget:
            for big in ((2 ** 31, 1), (2 ** 30, 2), (1, 2 ** 31), (2 ** 16, 2 ** 15), (3, 2 ** 63)):
                add(f"dummy-{big[0]}x{big[1]}", e, EINVAL, T_ROWS2, a=DUMMY, b=DUMMY, out=DUMMY, sets=1, batch=big[0], terms=big[1])
            add("batch0-terms-2^31", e, EINVAL, T_ROWS2, batch=0, terms=2 ** 31)
    e = "tn_poly_dot_hat_dev"
    for keep in (2, -1):
        add(f"out-prepared-{keep}", e, EINVAL, T_KEEP, out_prepared=keep)
    add("out-prepared-2-terms-0", e, EINVAL, T_TERMS, out_prepared=2, terms=0)
    add("out-prepared-2-rows-2^31", e, EINVAL, T_KEEP, out_prepared=2, batch=2 ** 31)

    # ---- the gadget calls: what both ask of (terms, base_log, flags) ----
    for e in ("tn_poly_gadget_dot_prepared_dev", "tn_gadget_decompose_dev"):
        add("balanced-ok", e, flags=1)
        add("gadget-terms-0", e, EINVAL, T_TERMS, terms=0)
        add("base-log-0", e, EINVAL, T_BASE, base_log=0)
        add("base-log-k", e, EINVAL, T_BASE, base_log=k)
        add("base-log-64", e, EINVAL, T_BASE, terms=1, sets=1, base_log=64)
        add("base-log-k-1-ok", e, base_log=k - 1)
        add("shift-66", e, EINVAL, T_SHIFT, terms=4, base_log=22)
        add("shift-64", e, EINVAL, T_SHIFT, terms=65, base_log=1)
        add("flag-2", e, EINVAL, T_FLAG, terms=2, base_log=30, flags=2)
        add("flag-high-bit", e, EINVAL, T_FLAG, terms=2, base_log=30, flags=0x80000001)
        add("flag-2-terms-0", e, EINVAL, T_TERMS, terms=0, flags=2)
        for big in ((2 ** 31, 1, w), (2 ** 30, 2, w), (2 ** 26, 32, 2), (2 ** 25, 64, 1)):
            add(f"dummy-{big[0]}x{big[1]}", e, EINVAL, T_ROWS2, a=DUMMY, b=DUMMY, out=DUMMY, sets=1, batch=big[0], terms=big[1], base_log=big[2])
    e = "tn_gadget_decompose_dev"
    add("ok", e)
    for plan in (GENERAL, OMEGA):
        add(f"{plan}-plan-ok", e, plan=plan)
    add("null-plan", e, EINVAL, T_PLAN, plan=NULL)
    add("null-a", e, EINVAL, T_BUFFER, a=None)
    add("null-digits", e, EINVAL, T_BUFFER, out=None)
    add("batch0-null", e, a=None, out=None, batch=0, terms=3, base_log=min(20, w), launches=False)
    add("digits-is-a", e, EINVAL, T_OVERLAP_THE, out=("A", 0))
    add("digits-last-row-is-first-of-a", e, EINVAL, T_OVERLAP_THE, out=("A", 1 - batch * terms))
    add("digits-first-row-is-last-of-a", e, EINVAL, T_OVERLAP_THE, out=("A", batch - 1))
    add("digits-just-past-a", e, out=("A", batch))

    # ---- synthetic rows and their digests ----
    e = "tn_fill_lcg_dev"
    add("ok", e)
    add("null-plan", e, EINVAL, T_ARGUMENT, plan=NULL)
    add("null-dst", e, EINVAL, T_ARGUMENT, out=None)
    add("batch0-null", e, out=None, batch=0)
    add("rows-2^32", e, EINVAL, T_WIDE, batch=2 ** 32)
    add("rows-2^32-null-dst", e, EINVAL, T_ARGUMENT, batch=2 ** 32, out=None)       # the pointers are looked at first
    e = "tn_checksum_rows_dev"
    add("ok", e)
    add("null-plan", e, EINVAL, T_ARGUMENT, plan=NULL)
    add("null-src", e, EINVAL, T_ARGUMENT, a=None)
    add("null-out", e, EINVAL, T_ARGUMENT, out=None)
    add("batch0-null", e, a=None, out=None, batch=0)
    add("rows-2^32", e, EINVAL, T_WIDE, batch=2 ** 32)
    assert len({c.id for c in rows}) == len(rows)
    return rows


def address(place, base, row_bytes):
    """The address a row's pointer stands for, the arena starting at `base`."""
    if place is None:
        return None
    if place == DUMMY:
        return 4096
    buffer, row = place
    assert 0 <= FIRST_ROW[buffer] + row < ARENA_ROWS
    return base + (FIRST_ROW[buffer] + row) * row_bytes


def c_arguments(case, base, row_bytes):
    """The arguments of the C entry point after the plan and before the stream, in the order of include/tinyntt.h."""
    g = case.args
    a, b, out = (address(g[x], base, row_bytes) for x in ("a", "b", "out"))
    e = case.entry
    if e in ("tn_poly_mult_dev", "tn_cyclic_poly_mult_dev"):
        return [a, b, out, g["batch"], 0]                                          # variant: TN_VARIANT_AUTO
    if e in ("tn_ntt_forward_dev", "tn_ntt_inverse_dev", "tn_twisted_ntt_forward_dev"):
        return [a, out, g["batch"], 0]
    if e in ("tn_schoolbook_dev", "tn_pointwise_mul_dev"):
        return [a, b, out, g["batch"]]
    if e in ("tn_prepare_dev", "tn_unprepare_dev"):
        return [a, out, g["batch"]]
    if e == "tn_poly_mult_prepared_dev":
        return [a, b, g["sets"], out, g["batch"]]
    if e == "tn_poly_dot_prepared_dev":
        return [a, b, g["sets"], out, g["batch"], g["terms"]]
    if e == "tn_poly_dot_hat_dev":
        return [a, b, g["sets"], out, g["batch"], g["terms"], g["out_prepared"]]
    if e == "tn_gadget_decompose_dev":
        return [a, out, g["batch"], g["terms"], g["base_log"], g["flags"]]
    if e == "tn_poly_gadget_dot_prepared_dev":
        return [a, b, g["sets"], out, g["batch"], g["terms"], g["base_log"], g["flags"]]
    if e == "tn_fill_lcg_dev":
        return [out, g["batch"], 1, 2]                                             # seed0, seed_stride
    if e == "tn_checksum_rows_dev":
        return [a, out, g["batch"]]
    raise KeyError(e)


def emu_check(lib, entry, view, a, b, out, sets=1, batch=1, terms=1, out_prepared=0, base_log=1, flags=0):
    """emu_api_check (tests/emu/emu_kernels.cpp): the entry point's own list of checks, on the CPU.  view: (n, elem_bytes,
    has_fused, omega_only, q), n = 0 for a NULL plan; a, b, out: addresses or None.  Returns (status, text, goes on to a launch)."""
    vp, sz, ci, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    lib.emu_api_check.argtypes = [ctypes.c_char_p, u32, ci, ci, ci, ctypes.c_uint64, vp, vp, vp, sz, sz, sz, ci, u32, u32, ctypes.POINTER(ci),
                                  ctypes.c_char_p, sz]
    msg, launch = ctypes.create_string_buffer(256), ci(-1)
    st = lib.emu_api_check(entry.encode(), *view, a, b, out, sets, batch, terms, out_prepared, base_log, flags, ctypes.byref(launch), msg, 256)
    assert st >= 0, entry
    return st, msg.value.decode(), bool(launch.value)


def emu_case(lib, case, n, elem_bytes, q, base=1 << 32):
    """One row of the table through emu_check, the arena standing at `base` (no memory is read)."""
    view = {FUSED: (n, elem_bytes, 1, 0, q), GENERAL: (n, elem_bytes, 0, 0, q), OMEGA: (n, elem_bytes, 0, 1, q), NULL: (0, 0, 0, 0, 0)}[case.plan]
    g = case.args
    a, b, out = (address(g[x], base, n * elem_bytes) for x in ("a", "b", "out"))
    return emu_check(lib, case.entry, view, a, b, out, g["sets"], g["batch"], g["terms"], g["out_prepared"], g["base_log"], g["flags"])
