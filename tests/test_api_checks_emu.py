"""The argument checks of the device entry points (tiny_ntt_amd/csrc/api_checks.h) on the CPU: emu_api_check runs, for an entry
point's name, the very list of steps capi.cpp runs before its launch.  No pointer is read, so any address will do."""
import pytest

import api_cases
import emu_library
from api_cases import EINVAL, OK
from conftest import PARAMS

GEOMETRIES = {tag: (PARAMS[tag][0], 4 if PARAMS[tag][1] < 2 ** 31 else 8, PARAMS[tag][1]) for tag in ("P256", "P4096_60")}
BATCH, TERMS = 5, 2                                         # the sizes tests/test_gpu_api_cases.py uses on the device
ENTRIES = sorted({c.entry for c in api_cases.cases(BATCH, TERMS, 60)})


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("tag", GEOMETRIES)
def test_every_row_of_the_table_gives_its_status_and_text(tag, entry):
    n, elem_bytes, q = GEOMETRIES[tag]
    lib = emu_library.load()
    table = [c for c in api_cases.cases(BATCH, TERMS, q.bit_length()) if c.entry == entry]
    assert table
    wrong = []
    for c in table:
        for base in (1 << 32, 0):                           # the second arena begins at address 0: pointers as small as they get
            st, text, launches = api_cases.emu_case(lib, c, n, elem_bytes, q, base)
            if (st, launches) != (c.status, c.launches) or (c.text is not None and text != c.text):
                wrong.append((c.id, base, st, text, launches))
    assert not wrong, wrong


# ---- overlap = the byte ranges intersect, by brute force --------------------------------------
N, WORD, Q, W = 4, 4, 7681, 4                               # the smallest plan: rows of 16 bytes; 2^W < Q
ROW = N * WORD
VIEW = (N, WORD, 1, 0, Q)
FAR = 1 << 40                                               # where the operand that is not under test lies
OFFSETS = range(-4 * ROW, 7 * ROW + 1, ROW // 2)            # every row offset -4 .. +7 and the half rows between them


def intersects(x, xbytes, y, ybytes):
    return bool(set(range(x, x + xbytes)) & set(range(y, y + ybytes)))


def shapes():
    """(entry, sets or None, out rows, rows of a, rows of b or None) as functions of (batch, terms)."""
    for e in ("tn_poly_mult_dev", "tn_cyclic_poly_mult_dev", "tn_schoolbook_dev"):
        yield e, None, lambda b, t: b, lambda b, t: b, lambda b, t: b
    for e in ("tn_ntt_forward_dev", "tn_ntt_inverse_dev", "tn_twisted_ntt_forward_dev", "tn_prepare_dev", "tn_unprepare_dev"):
        yield e, None, lambda b, t: b, lambda b, t: b, None
    yield "tn_gadget_decompose_dev", None, lambda b, t: b * t, lambda b, t: b, None
    for shared in (False, True):
        sets = (lambda b: 1) if shared else (lambda b: b)
        yield "tn_poly_mult_prepared_dev", sets, lambda b, t: b, lambda b, t: b, (lambda b, t: 1) if shared else (lambda b, t: b)
        brows = (lambda b, t: t) if shared else (lambda b, t: b * t)
        yield "tn_poly_dot_prepared_dev", sets, lambda b, t: b, lambda b, t: b * t, brows
        yield "tn_poly_dot_hat_dev", sets, lambda b, t: b, lambda b, t: b * t, brows
        yield "tn_poly_gadget_dot_prepared_dev", sets, lambda b, t: b, lambda b, t: b, brows


@pytest.mark.parametrize("shape", list(shapes()), ids=lambda s: s[0][3:-4] + ("" if s[1] is None else "-shared" if s[1](2) == 1 else "-sets"))
def test_overlap_is_the_intersection_of_the_byte_ranges(shape):
    entry, sets, out_rows, a_rows, b_rows = shape
    lib = emu_library.load()
    base = 1 << 20
    seen = set()
    for batch in (1, 2, 3):
        for terms in (1, 2, 3):
            kw = dict(sets=sets(batch) if sets else 1, batch=batch, terms=terms, base_log=W)
            for which in ("a", "b") if b_rows else ("a",):
                in_bytes = (a_rows if which == "a" else b_rows)(batch, terms) * ROW
                for off in OFFSETS:
                    out = base + off
                    a, b = (base, FAR) if which == "a" else (FAR, base)
                    st, text, launches = api_cases.emu_check(lib, entry, VIEW, a, b, out, **kw)
                    want = intersects(out, out_rows(batch, terms) * ROW, base, in_bytes)
                    assert (st == EINVAL and "overlap" in text and not launches) if want else (st == OK and launches), (batch, terms, which, off, st, text)
                    seen.add(want)
    assert seen == {False, True}


# ---- the row limit: 2^31 - 1 rows of the operand with the most rows ------------------------------
LIMIT_PAIRS = [(2 ** 31 - 2, 1), (2 ** 31 - 1, 1), (2 ** 31, 1), (1, 2 ** 31 - 2), (1, 2 ** 31 - 1), (1, 2 ** 31),
               (2 ** 16, 2 ** 15), (2 ** 15, 2 ** 16 - 1)]


def test_row_limit_holds_at_its_boundary():
    lib = emu_library.load()
    a, b, out = 1 << 44, 1 << 48, 1 << 52                       # 2^31 rows of 16 bytes apart, and more
    for entry in ENTRIES:
        if entry in ("tn_pointwise_mul_dev", "tn_fill_lcg_dev", "tn_checksum_rows_dev"):
            limit = 2 ** 32 - 1
            pairs = [(limit - 1, 1), (limit, 1), (limit + 1, 1)]
        elif "dot" in entry and "gadget" not in entry:
            limit, pairs = 2 ** 31 - 1, LIMIT_PAIRS
        elif "gadget" in entry:                                  # (terms - 1) * base_log < 64 keeps terms small
            limit, pairs = 2 ** 31 - 1, LIMIT_PAIRS[:3] + [(2 ** 25, 64), (2 ** 25 - 1, 64), (2 ** 26, 32)]
        else:
            limit, pairs = 2 ** 31 - 1, LIMIT_PAIRS[:3]
        for batch, terms in pairs:
            st, text, launches = api_cases.emu_check(lib, entry, VIEW, a, b, out, sets=1, batch=batch, terms=terms, base_log=1)
            if batch * terms <= limit:
                assert st == OK and launches, (entry, batch, terms, text)
            else:
                assert st == EINVAL and "too large" in text and not launches, (entry, batch, terms, text)
